"""Left-sited 4:2:0 chroma without a GPU (the mmhip_..._sited entry points, include/mmhip.h): the symbols and the header's
statement, the properties of the restatement tests/yuv_sited_reference.py and its agreement with the four centre-sited
restatements, what the siting does to a chroma stripe and to a round trip, csrc/mm_yuv.h compiled for the host in a
stand-alone program and compared bit for bit in both directions and at both depths, the stream header and its siting, and
every refusal of the new Python keywords, C calls and CLI options."""
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
from tests import yuv10_input_reference as R10I
from tests import yuv10_reference as R10
from tests import yuv_input_reference as RI
from tests import yuv_reference as R8
from tests import yuv_sited_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mathmap_amd", "csrc")
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
MODES = S.MODES
# the size table of the GPU tests of the four centre-sited converters
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (7, 3), (8, 2), (16, 2), (24, 4), (9, 2), (15, 6), (17, 9), (31, 33), (64, 8), (65, 7), (97, 61)]
HOST_SIZES = [(1, 1), (2, 1), (1, 2), (3, 5), (8, 2), (17, 9)]
NEW_SYMBOLS = ("mmhip_clip_to_yuv420_sited", "mmhip_clip_float_to_yuv420p10_sited", "mmhip_clip_from_yuv420_sited", "mmhip_clip_from_yuv420p10_sited",
               "mmhip_set_image_sequence_yuv420_host_sited", "mmhip_set_image_sequence_yuv420p10_host_sited", "mmhip_y4m_header_sited",
               "mmhip_y4m_stream_siting")


def err():
    return lib().mmhip_last_error().decode()


@pytest.fixture(autouse=True)
def the_sited_surface():
    """The restatement restates the library's statement: without the entry points it speaks for, no test here has a subject."""
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib(), name), name
    assert (_lib.MMHIP_YUV_SITING_CENTER, _lib.MMHIP_YUV_SITING_LEFT) == (0, 1)


def test_entry_points_exist_and_are_declared():
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib(), name) is not None, name
    header = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    shared = open(os.path.join(CSRC, "mm_yuv.h")).read()
    for name, value in (("MMHIP_YUV_SITING_CENTER", 0), ("MMHIP_YUV_SITING_LEFT", 1)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
        assert re.search(r"%s\s*=\s*%d\b" % (name.replace("MMHIP_", "MM_"), value), shared), name
    assert mm.api.YUV_SITINGS == {"center": 0, "left": 1} == S.SITING_IDS
    flat = " ".join(header.split())
    for declaration in (
            "int mmhip_clip_to_yuv420_sited(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width, "
            "int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst, int64_t dst_frame_stride, void *stream);",
            "int mmhip_clip_float_to_yuv420p10_sited(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, "
            "int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst, int64_t dst_frame_stride, void *stream);",
            "int mmhip_clip_from_yuv420_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames, "
            "int matrix, int range, int chroma, int siting, void *dst_rgba32, int64_t dst_frame_stride, void *stream);",
            "int mmhip_clip_from_yuv420p10_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames, "
            "int matrix, int range, int chroma, int siting, void *dst_float4, int64_t dst_frame_stride, void *stream);",
            "int mmhip_set_image_sequence_yuv420_host_sited(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width, "
            "int height, int num_frames, int matrix, int range, int chroma, int siting);",
            "int mmhip_set_image_sequence_yuv420p10_host_sited(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width, "
            "int height, int num_frames, int matrix, int range, int chroma, int siting);",
            "int mmhip_y4m_header_sited(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range, int bits, int siting);",
            "int mmhip_y4m_stream_siting(const char *buf, int len, int *siting);"):
        assert declaration in flat, declaration
    for phrase in ("2 cx - 1, 2 cx, 2 cx + 1 with the weights 1, 2, 1", "a column below 0 is column 0, a column at or above width is width - 1",
                   "a row at or above height is height - 1", "the weights sum to 8",
                   "Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^18) >> 19) + 128, 0, 255)",
                   "Cb = clamp(floor((cbr * Rs + cbg * Gs + cbb * Bs + 2^21) / 2^22) + 512, 0, 1023)", "[-2 143 256 608, 2 147 450 912]", "32 736 below 2^31", "computed in int64",
                   "grey gives 128 and 512 exactly", "col(i) = 3 * C[cy][i] + C[ny][i]", "r = min(cx + 1, cw - 1)", "C' = (4 * col(cx) + 8) >> 4",
                   "C' = (2 * col(cx) + 2 * col(r) + 8) >> 4", "S = 2 * col(cx) + 2 * col(r)", "the weights sum to 16",
                   "MMHIP_YUV_CHROMA_REPLICATE ignores the siting", "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not N",
                   "C420mpeg2 in place of C420jpeg", "Y4M has no tag for the siting of a 10-bit stream", "C420paldv", "is not modelled",
                   "tests/yuv_sited_reference.py"):
        assert phrase in flat, phrase
    for name in ("mm_yuv_chroma_left", "mm_yuv10_chroma_left", "mm_yuv_chroma_blend_left", "mm_yuv10_chroma_blend16_left", "mm_yuv_frame_host_sited",
                 "mm_yuv10_frame_host_sited", "mm_yuv_to_rgba_frame_host_sited", "mm_yuv10_to_float_frame_host_sited", "int64_t"):
        assert name in shared, name
    for source, kernel in (("clip_yuv.hip", "k_rgba8_to_yuv420_clip"), ("clip_yuv10.hip", "k_float_to_yuv420p10_clip"),
                           ("clip_yuv_in.hip", "k_yuv420_to_rgba_clip"), ("clip_yuv10_in.hip", "k_yuv420p10_to_float_clip")):
        text = open(os.path.join(CSRC, source)).read()
        assert kernel in text and "MM_YUV_SITING_LEFT" in text and "int SITING = MM_YUV_SITING_CENTER" in text, source
        assert "__shared__" not in text, source                                        # nothing is staged through LDS
    for name in ("set_image_yuv420", "set_image_yuv420p10", "clip_to_yuv420", "clip_float_to_yuv420p10", "clip_from_yuv420", "clip_from_yuv420p10"):
        assert inspect.signature(getattr(mm.api.Invocation, name)).parameters["chroma_siting"].default == "center", name
    assert inspect.signature(mm.api.Invocation.render_clip).parameters["chroma_siting"].default is None
    for name in ("y4m_header", "write_y4m"):
        assert inspect.signature(getattr(mm.api, name)).parameters["chroma_siting"].default == "center", name
    # what the readers return is what they returned
    assert len(mm.api.y4m_parse_header(b"YUV4MPEG2 W8 H6 C420mpeg2\n")) == 5 and len(mm.api.y4m_parse_stream_header(b"YUV4MPEG2 W8 H6 C420mpeg2\n")) == 6


# ---- consequences of the statement ----

def test_the_weights_sum_to_8_and_16():
    assert 2 * sum(S.OUT_WEIGHTS) == 8
    assert all(sum(pair) * 4 == 16 for pair in S.IN_WEIGHTS.values())
    ones = np.ones((5, 7, 3), np.int64)
    assert (S.left_sums(ones) == 8).all()                                   # every sample, the clamped edges included
    assert (S.left_seen16(np.ones((3, 4), np.int64), 7, 5) == 16).all()


@pytest.mark.parametrize("mode", MODES, ids="-".join)
def test_grey_frames_have_chroma_128_and_512(mode):
    w, h = 7, 5
    for v in (0, 1, 16, 127, 128, 200, 235, 255):
        _, cb, cr = S.planes8(np.full((h, w, 4), v, np.uint8), mode, "left")
        assert (cb == 128).all() and (cr == 128).all(), (mode, v)
    for v in (0.0, 1e-6, 0.25, 0.5, 0.7071, 1.0, 7.0, -1.0):
        _, cb, cr = S.planes10(np.full((h, w, 4), v, np.float32), mode, "left")
        assert (cb == 512).all() and (cr == 512).all(), (mode, v)
    # and a grey payload comes back grey under either siting
    grey8 = np.concatenate([np.arange(w * h, dtype=np.uint8) + 60, np.full(2 * 4 * 3, 128, np.uint8)])
    a = S.rgba_frames(grey8, w, h, mode, "bilinear", "left")
    assert np.array_equal(a, RI.rgba_frames(grey8, w, h, mode, "bilinear")) and np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 1], a[..., 2])
    grey10 = np.concatenate([np.arange(w * h, dtype=np.uint16) * 20 + 64, np.full(2 * 4 * 3, 512, np.uint16)])
    b = S.float_frames(grey10, w, h, mode, "bilinear", "left")
    assert np.array_equal(b.view(np.uint32), R10I.float_frames(grey10, w, h, mode, "bilinear").view(np.uint32))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_centre_through_the_sited_restatement_is_the_old_restatements(size):
    w, h = size
    rng = np.random.default_rng(100 * w + h)
    rgba = rng.integers(0, 256, (2, h, w, 4), dtype=np.uint8)
    pixels = (rng.random((2, h, w, 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    yuv8 = rng.integers(0, 256, (2, R8.frame_bytes(w, h)), dtype=np.uint8)
    yuv10 = rng.integers(0, 1400, (2, R10.frame_samples(w, h))).astype(np.uint16)
    for mode in MODES:
        assert np.array_equal(S.frames8(rgba, mode, "center"), R8.frames(rgba, mode))
        assert np.array_equal(S.frames10(pixels, mode, "center"), R10.frames(pixels, mode))
        for chroma in S.CHROMAS:
            assert np.array_equal(S.rgba_frames(yuv8, w, h, mode, chroma, "center"), RI.rgba_frames(yuv8, w, h, mode, chroma))
            assert np.array_equal(S.float_frames(yuv10, w, h, mode, chroma, "center").view(np.uint32),
                                  R10I.float_frames(yuv10, w, h, mode, chroma).view(np.uint32))
        # replicate ignores the siting; luma does too
        assert np.array_equal(S.rgba_frames(yuv8, w, h, mode, "replicate", "left"), RI.rgba_frames(yuv8, w, h, mode, "replicate"))
        assert np.array_equal(S.float_frames(yuv10, w, h, mode, "replicate", "left").view(np.uint32),
                              R10I.float_frames(yuv10, w, h, mode, "replicate").view(np.uint32))
        assert np.array_equal(S.frames8(rgba, mode, "left")[:, :w * h], R8.frames(rgba, mode)[:, :w * h])
        assert np.array_equal(S.frames10(pixels, mode, "left")[:, :w * h], R10.frames(pixels, mode)[:, :w * h])


def test_left_siting_by_hand():
    """One row pair of 4 x 2, bt709 full: the sums by hand, the clamped columns at both edges, and the seen chroma."""
    rgba = np.zeros((2, 4, 4), np.uint8)
    rgba[:, 0] = (255, 0, 0, 9)
    rgba[:, 3] = (0, 0, 255, 9)
    sums = S.left_sums(rgba)
    # cx 0: columns 0, 0, 1 -> red weighs (1 + 2) * 2 rows; cx 1: columns 1, 2, 3 -> blue weighs 1 * 2 rows
    assert sums.tolist() == [[[6 * 255, 0, 0], [0, 0, 2 * 255]]]
    _, cb, cr = S.planes8(rgba, ("bt709", "full"), "left")
    assert cb[0, 0] == (-7509 * 1530 + 2 ** 18) // 2 ** 19 + 128 and cr[0, 0] == (32768 * 1530 + 2 ** 18) // 2 ** 19 + 128
    assert cb[0, 1] == (32768 * 510 + 2 ** 18) // 2 ** 19 + 128 and cr[0, 1] == (-3005 * 510 + 2 ** 18) // 2 ** 19 + 128
    # an odd width: the last block's right column is the last column again
    odd = np.zeros((1, 3, 3), np.int64)
    odd[0, 2] = 1
    assert S.left_sums(odd)[0, 1].tolist() == [2 * (2 + 1)] * 3 and S.left_sums(odd)[0, 0].tolist() == [0] * 3
    # in: even columns lie on their sample, odd ones half way to the next, the last odd one on its own again
    plane = np.array([[0, 160], [80, 240]])
    seen = S.left_seen16(plane, 4, 4)
    assert seen[0].tolist() == [0, 2 * 4 * 160, 16 * 160, 16 * 160]
    assert seen[1].tolist() == [4 * 80, 2 * 80 + 2 * (3 * 160 + 240), 4 * (3 * 160 + 240), 4 * (3 * 160 + 240)]
    assert S.seen8(plane, 4, 4, "bilinear", "left")[0].tolist() == [0, 80, 160, 160]


def test_the_ten_bit_bound_at_the_extreme_colours():
    """The statement's bound, by enumeration: over the corners of the cube of sums -- where a linear form has its extremes --
    k . sums and every partial sum of it, in any order, stays within +-4092 * 524 280, and the intermediate with its rounding
    term ends 32 736 below 2^31 at pure blue and pure red, full range.  (So no colour makes a signed 32-bit sum wrap with
    these tables; the margin is the one the centre form changes its scale to avoid, hence int64.)  The samples at the
    extremes are pinned: the restatement forms them with Python ints."""
    import itertools
    top = 8 * 65535
    lowest, highest = 0, 0
    for mode in MODES:
        _, _, cb_row, cr_row = R10.TABLES[mode]
        for row in (cb_row, cr_row):
            assert sum(row) == 0
            for corner in itertools.product((0, top), repeat=3):
                for order in itertools.permutations(range(3)):
                    partial = 0
                    for i in order:
                        partial += int(row[i]) * corner[i]
                        lowest, highest = min(lowest, partial), max(highest, partial)
                assert S.left_intermediate(corner, row) == partial
    assert (lowest, highest) == (-4092 * 524280, 4092 * 524280) == (-2145353760, 2145353760)
    assert highest + 2 ** 21 == 2 ** 31 - 32736 == 2147450912 and lowest + 2 ** 21 == -2143256608
    assert (highest + 2 ** 21) // 2 ** 22 == 511 and (lowest + 2 ** 21) // 2 ** 22 == -511
    assert 2 * (4092 * 4 * 65535 + 2 ** 20) == highest + 2 ** 21                        # twice the centre form's 1 073 725 456
    for mode in (("bt601", "full"), ("bt709", "full")):
        for colour, want in (((0.0, 0.0, 1.0), (1023, None)), ((1.0, 0.0, 0.0), (None, 1023)), ((1.0, 1.0, 0.0), (1, None)), ((0.0, 1.0, 1.0), (None, 1))):
            frame = np.zeros((2, 4, 4), np.float32)
            frame[..., :3] = colour
            assert S.left_sums(R10.quant(frame[..., :3])).max() == top
            _, cb, cr = S.planes10(frame, mode, "left")
            assert want[0] is None or (cb == want[0]).all(), (mode, colour, cb)
            assert want[1] is None or (cr == want[1]).all(), (mode, colour, cr)
            centre = R10.planes(frame, mode)
            assert np.array_equal(cb, centre[1]) and np.array_equal(cr, centre[2])          # one colour: the centre-sited samples


def stripe(at, w=16, h=4):
    """A grey frame with a vertical stripe of saturated orange, 2 pixels wide from column `at`."""
    frame = np.full((h, w, 4), 128, np.uint8)
    frame[:, at:at + 2, :3] = (230, 128, 26)
    return frame


def centroid(rgba):
    """Where the colour of the middle row lies: the mean column weighted by |R - B|."""
    row = rgba[rgba.shape[0] // 2].astype(np.int64)
    d = np.abs(row[:, 0] - row[:, 2])
    return float((np.arange(len(d)) * d).sum()) / float(d.sum())


# The largest code difference between a stripe frame and what comes back from out -> in, per (stripe column, out siting,
# in siting): measured with the restatement at bt709 limited, bilinear.
STRIPE_MAX = {(6, "left", "left"): 59, (6, "center", "center"): 29, (6, "left", "center"): 51, (6, "center", "left"): 59,
              (7, "left", "left"): 59, (7, "center", "center"): 57, (7, "left", "center"): 72, (7, "center", "left"): 59}


@pytest.mark.parametrize("at", [6, 7], ids=["even", "odd"])
def test_a_chroma_stripe_lands_on_its_own_columns(at):
    """Out and in again with one siting leaves the stripe's colour centred on its two columns, at + 0.5; written left-sited
    and read as centre-sited it moves half a pixel to the right (a quarter each way), the other way round half a pixel to
    the left.  The centroid tolerance: every returned code is within a code or two of the exact blend, over a support of at
    most 8 columns against a summed |R - B| of some 400.  The largest code difference is that of the 4:2:0 subsampling
    itself -- a stripe 2 pixels wide is a chroma sample and a half -- so the matched pairings do not exceed the worse of
    the two mixed ones, and no more is claimed of them."""
    mode = ("bt709", "limited")
    frame = stripe(at)
    h, w = frame.shape[:2]
    found, worst = {}, {}
    for out_siting in S.SITINGS:
        payload = S.frame8(frame, mode, out_siting)
        for in_siting in S.SITINGS:
            back = S.rgba_frames(payload, w, h, mode, "bilinear", in_siting)[0]
            found[out_siting, in_siting] = centroid(back)
            worst[out_siting, in_siting] = int(np.abs(back[..., :3].astype(np.int64) - frame[..., :3].astype(np.int64)).max())
            print("stripe at %d, out %s in %s: centroid %.4f, max difference %d" % (at, out_siting, in_siting, found[out_siting, in_siting],
                                                                                    worst[out_siting, in_siting]))
    assert abs(centroid(frame) - (at + 0.5)) < 1e-9
    for siting in S.SITINGS:
        assert abs(found[siting, siting] - (at + 0.5)) < 0.1, (siting, found)
    assert abs(found["left", "center"] - (at + 1.0)) < 0.1 and abs(found["center", "left"] - at) < 0.1, found
    for pair, value in worst.items():
        assert value == STRIPE_MAX[(at,) + pair], (at, pair, value)
    # "Must not exceed the mixed pairing" is read here as the worse of the two mixed pairings, which is weaker than either
    # alone: at the even column left/left (59) exceeds left -> centre (51) and equals centre -> left (59).  The figure is the
    # subsampling's own blur of a stripe a chroma sample and a half wide; what the siting does shows in the centroids above.
    mixed = max(worst["left", "center"], worst["center", "left"])
    assert worst["left", "left"] <= mixed and worst["center", "center"] <= mixed


# The largest distance of a sample after out -> in -> out from the sample after out, left siting both ways, replicate mode,
# over 200 000 seeded colours in gamut: measured with the restatement, per layout, depth and mode.  "blocks" is the frame
# of the 10-bit input test, 2 x 2 blocks of one colour each: the 1, 2, 1 filter reaches a column into the neighbouring
# block, replicate mode hands that mixture back as the block's colour and the second pass mixes again, so the samples
# move by what neighbouring colours differ by, not by a rounding.  "rows" gives every row pair one colour, which the
# filter leaves alone: there the samples come back within one code, as at centre siting.
ROUND_TRIP_MAX = {
    ("blocks", 10): {("bt601", "limited"): 141, ("bt601", "full"): 161, ("bt709", "limited"): 145, ("bt709", "full"): 165},
    ("blocks", 8): {("bt601", "limited"): 35, ("bt601", "full"): 40, ("bt709", "limited"): 36, ("bt709", "full"): 41},
    ("rows", 10): {("bt601", "limited"): 0, ("bt601", "full"): 1, ("bt709", "limited"): 1, ("bt709", "full"): 1},
    ("rows", 8): {("bt601", "limited"): 1, ("bt601", "full"): 1, ("bt709", "limited"): 1, ("bt709", "full"): 1},
}


def round_trip_frame(layout):
    """200 000 colours in gamut, seeded: float32 [h, w, 3]."""
    if layout == "blocks":
        blocks = np.random.default_rng(2024).random((250, 1600, 3), dtype=np.float32)           # 2 x 2-constant blocks, 500 x 3200
        return np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)
    rows = np.random.default_rng(2024).random((200000, 1, 3), dtype=np.float32)                 # constant row pairs, 400 000 x 4
    return np.repeat(np.repeat(rows, 2, axis=0), 4, axis=1)


@pytest.mark.parametrize("layout", ["blocks", "rows"])
@pytest.mark.parametrize("mode", MODES, ids="-".join)
def test_out_in_out_over_a_seeded_set(mode, layout):
    frame = round_trip_frame(layout)
    h, w = frame.shape[:2]
    first = S.frame10(frame, mode, "left")
    again = S.frame10(S.float_frames(first, w, h, mode, "replicate", "left")[0], mode, "left")
    worst10 = int(np.abs(again.astype(np.int64) - first.astype(np.int64)).max())
    bytes8 = np.rint(frame * np.float32(255)).astype(np.uint8)
    first8 = S.frame8(bytes8, mode, "left")
    again8 = S.frame8(S.rgba_frames(first8, w, h, mode, "replicate", "left")[0], mode, "left")
    worst8 = int(np.abs(again8.astype(np.int64) - first8.astype(np.int64)).max())
    print("out -> in -> out, left siting, %s, %s %s: max %d at 8 bits, %d at 10" % (layout, mode[0], mode[1], worst8, worst10))
    assert worst10 == ROUND_TRIP_MAX[layout, 10][mode] and worst8 == ROUND_TRIP_MAX[layout, 8][mode]


# ---- mm_yuv.h on the host ----

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mm_yuv.h"
// what in width height matrix range chroma siting out; what: 0 RGBA8 -> 8 bit, 1 float4 -> 10 bit, 2 8 bit -> words, 3 10 bit -> float4
template <class T>
static bool load(const char *name, std::vector<T> &v) {
    FILE *f = fopen(name, "rb");
    const bool ok = f && fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) fclose(f);
    return ok;
}
template <class T>
static bool save(const char *name, const std::vector<T> &v) {
    FILE *f = fopen(name, "wb");
    const bool ok = f && fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) fclose(f);
    return ok;
}
int main(int argc, char **argv) {
    if (argc != 10) return 2;
    const int what = atoi(argv[1]), w = atoi(argv[3]), h = atoi(argv[4]), matrix = atoi(argv[5]), range = atoi(argv[6]), chroma = atoi(argv[7]),
              siting = atoi(argv[8]);
    if (!mm_yuv_mode_known(matrix, range) || !mm_yuv_chroma_known(chroma) || !mm_yuv_siting_known(siting)) return 3;
    const size_t pixels = (size_t)w * h, samples = (size_t)mm_yuv_frame_bytes(w, h);
    if (what == 0) {
        std::vector<unsigned char> src(pixels * 4), dst(samples);
        if (!load(argv[2], src)) return 4;
        mm_yuv_frame_host_sited(MM_YUV_MODES[matrix][range], siting, src.data(), (int64_t)w * 4, w, h, dst.data());
        return save(argv[9], dst) ? 0 : 6;
    }
    if (what == 1) {
        std::vector<float> src(pixels * 4);
        std::vector<uint16_t> dst(samples);
        if (!load(argv[2], src)) return 4;
        mm_yuv10_frame_host_sited(MM_YUV10_MODES[matrix][range], siting, src.data(), (int64_t)w * 16, w, h, dst.data());
        return save(argv[9], dst) ? 0 : 6;
    }
    if (what == 2) {
        std::vector<unsigned char> src(samples);
        std::vector<uint32_t> dst(pixels);
        if (!load(argv[2], src)) return 4;
        mm_yuv_to_rgba_frame_host_sited(MM_YUV_RGBA_MODES[matrix][range], chroma, siting, src.data(), w, h, dst.data());
        return save(argv[9], dst) ? 0 : 6;
    }
    if (what == 3) {
        std::vector<uint16_t> src(samples);
        std::vector<float> dst(pixels * 4);
        if (!load(argv[2], src)) return 4;
        mm_yuv10_to_float_frame_host_sited(MM_YUV10_FLOAT_MODES[matrix][range], chroma, siting, src.data(), w, h, dst.data());
        return save(argv[9], dst) ? 0 : 6;
    }
    return 5;
}
"""
OUT_DTYPES = {0: np.uint8, 1: np.uint16, 2: np.uint32, 3: np.float32}


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitizers"])
def host_program(request):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="mm_yuv_sited_")
    open(os.path.join(d, "t.cpp"), "w").write(PROGRAM)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    exe = os.path.join(d, "t")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", CSRC, "-o", exe, os.path.join(d, "t.cpp")], check=True)

    def convert(what, data, w, h, mode, chroma="bilinear", siting="left"):
        np.ascontiguousarray(data).tofile(os.path.join(d, "in.bin"))
        r = subprocess.run([exe, str(what), os.path.join(d, "in.bin"), str(w), str(h), str(S.MATRIX_IDS[mode[0]]), str(S.RANGE_IDS[mode[1]]),
                            str(S.CHROMA_IDS[chroma]), str(S.SITING_IDS[siting]), os.path.join(d, "out.bin")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return np.fromfile(os.path.join(d, "out.bin"), OUT_DTYPES[what])
    yield convert
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("size", HOST_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_frames_are_the_restatements_bit_for_bit(host_program, size):
    w, h = size
    rng = np.random.default_rng(10 * w + h)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pixels = (rng.random((h, w, 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    yuv8 = rng.integers(0, 256, R8.frame_bytes(w, h), dtype=np.uint8)
    yuv10 = rng.integers(0, 65536, R10.frame_samples(w, h)).astype(np.uint16)
    for mode in MODES:
        for siting in S.SITINGS:
            assert np.array_equal(host_program(0, rgba, w, h, mode, siting=siting), S.frame8(rgba, mode, siting)), (size, mode, siting)
            assert np.array_equal(host_program(1, pixels, w, h, mode, siting=siting), S.frame10(pixels, mode, siting)), (size, mode, siting)
            for chroma in S.CHROMAS:
                got = host_program(2, yuv8, w, h, mode, chroma, siting)
                assert np.array_equal(got, RI.words(S.rgba_frames(yuv8, w, h, mode, chroma, siting)[0]).reshape(-1)), (size, mode, chroma, siting)
                got = host_program(3, yuv10, w, h, mode, chroma, siting)
                assert np.array_equal(got.view(np.uint32), S.float_frames(yuv10, w, h, mode, chroma, siting)[0].reshape(-1).view(np.uint32)), \
                    (size, mode, chroma, siting)


def test_the_host_frames_over_every_sample_value(host_program):
    """All of 0 .. 65535 as 10-bit input samples and as quantised channels, all bytes at 8 bits, on frames whose neighbouring
    columns differ: 512 x 2 pixels hold 1024 + 2 * 256 samples."""
    w, h = 512, 2
    rng = np.random.default_rng(7)
    every16 = rng.permutation(65536).astype(np.uint16)
    for start in range(0, 65536, 1536):                        # every value once as luma or chroma
        block = np.resize(every16[start:start + 1536], 1536)
        yuv10 = np.concatenate([block[:1024], block[1024:1280], block[1280:1536]])
        for mode in (("bt709", "limited"), ("bt601", "full")):
            got = host_program(3, yuv10, w, h, mode, "bilinear", "left")
            assert np.array_equal(got.view(np.uint32), S.float_frames(yuv10, w, h, mode, "bilinear", "left")[0].reshape(-1).view(np.uint32)), (start, mode)
    # every quantised channel value: q / 65535 quantises back to q
    q = rng.permutation(65536).astype(np.float32) / np.float32(65535)
    pixels = np.zeros((128, 512, 4), np.float32)
    pixels[..., 0], pixels[..., 1], pixels[..., 2] = q.reshape(128, 512), np.roll(q, 17).reshape(128, 512), np.roll(q, 4711).reshape(128, 512)
    assert set(R10.quant(pixels[..., 0]).reshape(-1).tolist()) == set(range(65536))
    every8 = np.stack([rng.permutation(256), rng.permutation(256), rng.permutation(256), rng.permutation(256)], axis=-1).astype(np.uint8).reshape(2, 128, 4)
    for start in (0, 128):                                     # every byte as chroma too
        planes = rng.permutation(256)[start:start + 128]
        yuv8 = np.concatenate([rng.permutation(256), planes[:64], planes[64:]]).astype(np.uint8)
        for mode in MODES:
            got = host_program(2, yuv8, 128, 2, mode, "bilinear", "left")
            assert np.array_equal(got, RI.words(S.rgba_frames(yuv8, 128, 2, mode, "bilinear", "left")[0]).reshape(-1)), mode
    for mode in MODES:
        assert np.array_equal(host_program(1, pixels, 512, 128, mode), S.frame10(pixels, mode, "left")), mode
        assert np.array_equal(host_program(0, every8, 128, 2, mode), S.frame8(every8, mode, "left")), mode


def test_the_host_frame_at_the_extreme_colours(host_program):
    """Columns of blue, red, yellow, cyan, white and black: k . sums reaches both ends of its range, 32 736 below 2^31 with
    the rounding term."""
    colours = np.array([(0, 0, 1), (0, 0, 1), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 1, 1), (1, 1, 0), (1, 1, 0), (1, 1, 0), (0, 0, 0),
                        (0, 1, 1), (0, 1, 1), (0, 1, 1), (1, 1, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0)], np.float32)
    pixels = np.zeros((3, len(colours), 4), np.float32)
    pixels[..., :3] = colours[None]
    for mode in MODES:
        want = S.frame10(pixels, mode, "left")
        assert np.array_equal(host_program(1, pixels, len(colours), 3, mode), want), mode
    _, cb, cr = S.planes10(pixels, ("bt709", "full"), "left")
    assert cb[0, 0] == 1023 and cr[0, 2] == 1023 and cb[0, 4] == 1 and cr[0, 6] == 1          # blue, red, yellow, cyan


# ---- the stream header ----

def test_y4m_header_sited_lines():
    def line(w, h, num, den, rng, bits, siting, cap=160):
        buf = C.create_string_buffer(cap)
        n = lib().mmhip_y4m_header_sited(buf, cap, w, h, num, den, rng, bits, siting)
        return None if n < 0 else buf.raw[:n]
    for rng_name, rng in (("limited", 0), ("full", 1)):
        assert line(17, 9, 30000, 1001, rng, 8, 0) == mm.api.y4m_header(17, 9, (30000, 1001), rng_name) == R8.y4m_header(17, 9, (30000, 1001), rng_name)
        assert line(17, 9, 24, 1, rng, 10, 0) == mm.api.y4m_header(17, 9, (24, 1), rng_name, "yuv420p10") == R10.y4m_header(17, 9, (24, 1), rng_name)
        assert line(17, 9, 24, 1, rng, 10, 1) == R10.y4m_header(17, 9, (24, 1), rng_name)              # no tag for it
        assert line(17, 9, 24, 1, rng, 8, 1) == b"YUV4MPEG2 W17 H9 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=%s\n" % rng_name.upper().encode()
        for bits in (8, 10):
            for siting in S.SITINGS:
                fmt = "yuv420p10" if bits == 10 else "yuv420p"
                assert mm.api.y4m_header(8, 6, 25, rng_name, fmt, chroma_siting=siting) == S.y4m_header(8, 6, (25, 1), rng_name, bits, siting)
    assert line(8, 6, 25, 1, 0, 12, 0) is None and err() == "y4m_header_sited: bits must be 8 or 10, not 12"
    assert line(8, 6, 25, 1, 0, 8, 2) is None and err() == "y4m_header_sited: siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
    assert line(0, 6, 25, 1, 0, 8, 1) is None and err() == "y4m_header_sited: width and height must be at least 1"
    assert line(8, 6, 0, 1, 0, 8, 1) is None and err() == "y4m_header_sited: fps_num and fps_den must be at least 1"
    assert line(8, 6, 25, 1, 2, 8, 1) is None and err() == "y4m_header_sited: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not 2"
    assert line(8, 6, 25, 1, 0, 8, 1, cap=20) is None and err() == "y4m_header_sited: the buffer holds 20 bytes, the header needs 61"
    with pytest.raises(ValueError, match="chroma_siting must be one of center, left, not 'top'"):
        mm.api.y4m_header(8, 6, chroma_siting="top")


def test_y4m_chroma_siting_over_every_accepted_tag(tmp_path):
    siting = mm.api.y4m_chroma_siting
    assert siting(b"YUV4MPEG2 W8 H6 C420mpeg2\n") == "left" and siting(b"YUV4MPEG2 W8 H6 F24:1 Ip C420mpeg2 XCOLORRANGE=FULL\nFRAME\n") == "left"
    for tag in (b"", b" C420", b" C420jpeg", b" C420paldv", b" C420p10"):
        assert siting(b"YUV4MPEG2 W8 H6" + tag + b"\n") == "center", tag
    assert siting(bytearray(mm.api.y4m_header(8, 6, chroma_siting="left"))) == "left" and siting(memoryview(mm.api.y4m_header(8, 6))) == "center"
    assert siting(mm.api.y4m_header(8, 6, pixel_format="yuv420p10", chroma_siting="left")) == "center"
    path = str(tmp_path / "left.y4m")
    mm.api.write_y4m(path, np.zeros((1, 72), np.uint8), 8, 6, chroma_siting="left")
    assert siting(path) == "left" and siting(tmp_path / "left.y4m") == "left"
    for line, word in ((b"YUV4MPEG2 W8 H6 C444\n", "colour space `C444' is not 4:2:0 of 8 or 10 bits (C420jpeg, C420mpeg2, C420paldv, C420 or C420p10)"),
                       (b"YUV4MPEG2 W8 H6 C420p12\n", "colour space `C420p12'"), (b"YUV4MPEG2 W8 H6 It\n", "interlaced"),
                       (b"YUV4MPEG W8 H6\n", "magic word"), (b"YUV4MPEG2 W8\n", "W and H"), (b"YUV4MPEG2 W8 H6 F25\n", "frame rate"),
                       (b"YUV4MPEG2 W8 H6 C420mpeg2", "no newline"), (b"YUV4MPEG2 W8 H6 Q1\n", "header tag `Q1'")):
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            siting(line)
        assert str(e.value).startswith("y4m_stream_siting: "), str(e.value)
        with pytest.raises(ValueError) as other:
            mm.api.y4m_parse_stream_header(line)
        assert str(other.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]                  # its words
    line = b"YUV4MPEG2 W8 H6 C420mpeg2\n"
    assert lib().mmhip_y4m_stream_siting(line, len(line), None) == 0
    # the parsers return what they returned, whatever the tag
    assert mm.api.y4m_parse_header(line) == (8, 6, (25, 1), None, len(line))
    assert mm.api.y4m_parse_stream_header(line) == (8, 6, (25, 1), None, len(line), "yuv420p")


def test_write_y4m_with_a_siting(tmp_path):
    w, h, n = 5, 3, 2
    flat = np.random.default_rng(2).integers(0, 256, (n, R8.frame_bytes(w, h)), dtype=np.uint8)
    deep = np.random.default_rng(3).integers(0, 1024, (n, R10.frame_samples(w, h))).astype(np.uint16)
    data = io.BytesIO()
    mm.api.write_y4m(data, flat, w, h, fps=(24, 1), yuv_range="full", chroma_siting="left")
    want = b"YUV4MPEG2 W5 H3 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n" + b"".join(b"FRAME\n" + f.tobytes() for f in flat)
    assert data.getvalue() == want
    assert data.getvalue().replace(b"C420mpeg2", b"C420jpeg") == R8.y4m_file(flat, w, h, (24, 1), "full")
    path = str(tmp_path / "left.y4m")
    mm.api.write_y4m(path, flat, w, h, chroma_siting="left")
    yuv, gw, gh, fps, rng = mm.api.read_y4m(path)                                       # read as before: the tag is accepted
    assert np.array_equal(yuv, flat) and (gw, gh, fps, rng) == (w, h, (25, 1), "limited")
    for siting in S.SITINGS:
        data = io.BytesIO()
        mm.api.write_y4m(data, deep, w, h, chroma_siting=siting)
        assert data.getvalue() == R10.y4m_file(deep, w, h)
    data = io.BytesIO()
    mm.api.write_y4m(data, flat, w, h, chroma_siting="center")
    assert data.getvalue() == R8.y4m_file(flat, w, h)
    with pytest.raises(ValueError, match="chroma_siting must be one of center, left, not 'mpeg2'"):
        mm.api.write_y4m(io.BytesIO(), flat, w, h, chroma_siting="mpeg2")


# ---- refusals ----

def test_python_argument_errors():
    """Refused before anything else is looked at (an invocation needs a GPU; the checks do not, so an unbound one will do)."""
    inv = mm.api.Invocation.__new__(mm.api.Invocation)
    inv.render_width, inv.render_height = 16, 8
    for bad in ("right", "Left", "centre", None, 1, ""):
        message = re.escape("chroma_siting must be one of center, left, not %r" % (bad,))
        with pytest.raises(ValueError, match=message):
            inv.set_image_yuv420("in", np.zeros((2, 192), np.uint8), 16, 8, chroma_siting=bad)
        with pytest.raises(ValueError, match=message):
            inv.set_image_yuv420p10("in", np.zeros((2, 192), np.uint16), 16, 8, chroma_siting=bad)
        with pytest.raises(ValueError, match=message):
            inv.clip_to_yuv420(0x1000, 0x2000, 2, chroma_siting=bad)
        with pytest.raises(ValueError, match=message):
            inv.clip_float_to_yuv420p10(0x1000, 0x2000, 2, chroma_siting=bad)
        with pytest.raises(ValueError, match=message):
            inv.clip_from_yuv420(0x1000, 0x2000, 2, chroma_siting=bad)
        with pytest.raises(ValueError, match=message):
            inv.clip_from_yuv420p10(0x1000, 0x2000, 2, chroma_siting=bad)
        if bad is not None:
            for pixel_format in ("yuv420p", "yuv420p10"):
                with pytest.raises(ValueError, match=message):
                    inv.render_clip(num_frames=2, pixel_format=pixel_format, chroma_siting=bad)
    for siting in ("center", "left", "up"):
        with pytest.raises(ValueError, match="render_clip: chroma_siting goes with pixel_format"):
            inv.render_clip(num_frames=2, chroma_siting=siting)
    # the other refusals of the setters stand in front of a good siting as they did
    with pytest.raises(ValueError, match="chroma must be one of bilinear, replicate"):
        inv.set_image_yuv420("in", np.zeros((2, 192), np.uint8), 16, 8, chroma="nearest", chroma_siting="left")
    with pytest.raises(ValueError, match=r"set_image_yuv420: uint8 \[N, 192\] for frames of 16 x 8"):
        inv.set_image_yuv420("in", np.zeros((2, 191), np.uint8), 16, 8, chroma_siting="left")
    with pytest.raises(ValueError, match="render_clip: pixel_format is not combined with floatmap"):
        inv.render_clip(num_frames=2, pixel_format="yuv420p", chroma_siting="left", floatmap=True)


def test_the_out_calls_refuse_bad_arguments_by_name():
    """The converters' checks come before the invocation is looked at: without one, a call that passes them all says so."""
    for name, bpp, dst_name, frame in (("clip_to_yuv420_sited", 4, "src_rgba and dst", 192), ("clip_float_to_yuv420p10_sited", 16, "src and dst", 384)):
        call = getattr(lib(), "mmhip_" + name)

        def refused(src=0x1000, row=16 * bpp, stride=16 * bpp * 8, w=16, h=8, first=0, last=8, n=2, matrix=1, rng=0, siting=1, dst=0x2000, dst_stride=frame):
            assert call(None, C.c_void_p(src), row, stride, w, h, first, last, n, matrix, rng, siting, C.c_void_p(dst), dst_stride, None) == -1
            return err()
        who = name + ": "
        assert refused() == refused(siting=0) == who + "no invocation"
        assert refused(siting=2) == who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert refused(siting=-1) == who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not -1"
        assert refused(w=0) == who + "width and height must be at least 1, not 0 x 8"
        assert refused(n=0) == who + "num_frames must be at least 1"
        assert refused(n=65536) == who + "more than 65535 frames in one call (65536); convert the clip in groups"
        assert refused(matrix=2) == who + "matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not 2"
        assert refused(rng=2, siting=2) == who + "range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not 2"          # in that order
        assert refused(siting=2, first=1) == who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert refused(first=8) == who + "rows [8, 8) are not rows of a frame of 8"
        assert refused(first=1) == who + "first_row must be even, not 1"
        assert refused(last=7) == who + "last_row must be even or equal to height, not 7 of 8"
        assert refused(src=0) == refused(dst=0) == who + dst_name + " must be device pointers"
        assert refused(row=16 * bpp - 4) == who + "src_row_stride %d is smaller than one row (%d bytes)" % (16 * bpp - 4, 16 * bpp)
        assert refused(dst_stride=frame - 2) == who + "dst_frame_stride %d is smaller than one frame (%d bytes)" % (frame - 2, frame)
    # the same calls without the siting keep their own names
    assert lib().mmhip_clip_to_yuv420(None, C.c_void_p(0x1000), 64, 512, 16, 8, 0, 8, 2, 1, 0, C.c_void_p(0x2000), 192, None) == -1
    assert err() == "clip_to_yuv420: no invocation"
    assert lib().mmhip_clip_float_to_yuv420p10(None, C.c_void_p(0x1000), 256, 2048, 16, 8, 0, 8, 2, 1, 2, C.c_void_p(0x2000), 384, None) == -1
    assert err() == "clip_float_to_yuv420p10: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not 2"


def test_the_in_calls_refuse_bad_arguments_by_name():
    for name, frame, dst_name, out in (("clip_from_yuv420_sited", 192, "src_yuv and dst_rgba32", 512), ("clip_from_yuv420p10_sited", 384, "src_yuv and dst_float4", 2048)):
        call = getattr(lib(), "mmhip_" + name)

        def refused(src=0x1000, stride=frame, w=16, h=8, n=2, matrix=1, rng=0, chroma=0, siting=1, dst=0x2000, dst_stride=out):
            assert call(None, C.c_void_p(src), stride, w, h, n, matrix, rng, chroma, siting, C.c_void_p(dst), dst_stride, None) == -1
            return err()
        who = name + ": "
        assert refused() == refused(siting=0) == refused(chroma=1) == who + "no invocation"
        assert refused(siting=2) == refused(siting=2, chroma=1) == who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert refused(w=0) == who + "width and height must be at least 1, not 0 x 8"
        assert refused(n=0) == who + "num_frames must be at least 1"
        assert refused(n=65536) == who + "more than 65535 frames in one call (65536); convert the clip in groups"
        assert refused(matrix=-1) == who + "matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not -1"
        assert refused(rng=2) == who + "range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not 2"
        assert refused(chroma=2, siting=2) == who + "chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not 2"
        assert refused(siting=2, src=0) == who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert refused(src=0) == refused(dst=0) == who + dst_name + " must be device pointers"
        assert refused(stride=frame - 2) == who + "src_frame_stride %d is smaller than one frame (%d bytes)" % (frame - 2, frame)
        assert refused(dst_stride=out - 16) == who + "dst_frame_stride %d is smaller than one frame (%d bytes)" % (out - 16, out)
    assert lib().mmhip_clip_from_yuv420(None, C.c_void_p(0x1000), 192, 16, 8, 2, 1, 0, 2, C.c_void_p(0x2000), 512, None) == -1
    assert err() == "clip_from_yuv420: chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not 2"
    # the host setters: their own refusals under their own names, with nothing allocated
    assert lib().mmhip_set_image_sequence_yuv420_host_sited(None, 0, None, 192, 16, 8, 2, 1, 0, 0, 1) == -1
    assert err() == "set_image_sequence_yuv420_host_sited: no payloads"
    assert lib().mmhip_set_image_sequence_yuv420_host_sited(None, 0, C.c_void_p(0x1000), 192, 16, 8, 2, 1, 0, 0, 2) == -1
    assert err() == "clip_from_yuv420_sited: siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
    assert lib().mmhip_set_image_sequence_yuv420_host_sited(None, 0, C.c_void_p(0x1000), 190, 16, 8, 2, 1, 0, 0, 1) == -1
    assert err() == "set_image_sequence_yuv420_host_sited: frame_stride 190 is smaller than one frame (192 bytes)"
    assert lib().mmhip_set_image_sequence_yuv420p10_host_sited(None, 0, None, 384, 16, 8, 2, 1, 0, 0, 1) == -1
    assert err() == "set_image_sequence_yuv420p10_host_sited: the pixels are a null pointer"
    assert lib().mmhip_set_image_sequence_yuv420_host(None, 0, None, 192, 16, 8, 2, 1, 0, 0) == -1
    assert err() == "set_image_sequence_yuv420_host: no payloads"


def test_cli_help_and_argument_errors(tmp_path):
    p = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    for phrase in ("--chroma-siting=SITING", "center (default", "C420mpeg2", "--input-chroma-siting=SITING", "auto (left", "C420p10 has no tag for it",
                   "replicate chroma ignores it", "(C420jpeg chroma siting)"):
        assert phrase in p.stdout, phrase
    one = "filter f (image in) in(xy, frame) end"
    plain = "filter f () rgba:[t, 0, 0, 1] end"
    good = str(tmp_path / "good.y4m")
    mm.api.write_y4m(good, np.full((2, R8.frame_bytes(8, 6)), 128, np.uint8), 8, 6, chroma_siting="left")
    out, png = str(tmp_path / "out.y4m"), str(tmp_path / "out.png")
    cases = [(["--chroma-siting=top", "-s", "8x8"], plain, out, "--chroma-siting takes center or left"),
             (["--chroma-siting=", "-s", "8x8"], plain, out, "--chroma-siting takes center or left"),
             (["--chroma-siting=auto", "-s", "8x8"], plain, out, "--chroma-siting takes center or left"),
             (["--chroma-siting=left", "-s", "8x8"], plain, png, "--chroma-siting goes with an output file name ending in .y4m (or -)"),
             (["--input-chroma-siting=right", "-Din=" + good], one, out, "--input-chroma-siting takes center, left or auto"),
             (["--input-chroma-siting=", "-Din=" + good], one, out, "--input-chroma-siting takes center, left or auto"),
             (["--input-chroma-siting=left", "-Din=in.png"], one, out, "--input-chroma-siting goes with an input image whose file name ends in .y4m (or is -)"),
             (["--input-chroma-siting=auto", "-s", "8x8"], plain, out, "--input-chroma-siting goes with an input image")]
    for extra, src, target, word in cases:
        p = subprocess.run([CLI] + extra + [src, target], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("Error:") and word in p.stderr, (extra, p.stderr)
    assert not os.path.exists(out) and not os.path.exists(png)
