"""Left-sited 4:2:0 chroma on the GPU (the mmhip_..._sited entry points: the SITING = MM_YUV_SITING_LEFT instantiations of
k_rgba8_to_yuv420_clip, k_float_to_yuv420p10_clip, k_yuv420_to_rgba_clip and k_yuv420p10_to_float_clip).

The yardstick is tests/yuv_sited_reference.py.  Everything is compared bit for bit in whole sentinel-filled destination
buffers: in front of the first frame, between frames, beyond every plane and behind the last frame nothing may change."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import yuv10_reference as R10
from tests import yuv_reference as R8
from tests import yuv_sited_reference as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
SENTINEL = 0xA5
LEAD = 64                    # sentinel bytes in front of the first and behind the last frame (keeps the base 16-byte aligned)
PLAIN = "filter plain (image in) in(xy, frame) end"
BENT = "filter bent (image in) in(xy * 1.3 + xy:[0.11, -0.07], frame) end"
SWIRL = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (7, 3), (8, 2), (16, 2), (17, 9), (24, 6), (64, 8), (65, 9), (129, 5)]
MODES = S.MODES
DEPTHS = (8, 10)


def err():
    return lib().mmhip_last_error().decode()


@pytest.fixture(scope="module")
def inv():
    """Any invocation: the converters use its stream, its timing records and its counters, nothing else."""
    return mm.Filter("filter f () rgba:[t, 0, 0, 1] end").invoke(8, 8)


def device_filled(total):
    p = lib().mmhip_device_alloc(total)
    assert p
    fill = np.full(total, SENTINEL, np.uint8)
    assert lib().mmhip_copy_to_device(C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), total) == 0
    return p


def upload(array):
    array = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    p = lib().mmhip_device_alloc(array.nbytes)
    assert p
    assert lib().mmhip_copy_to_device(C.c_void_p(p), array.ctypes.data_as(C.c_void_p), array.nbytes) == 0
    return p


def device_read(p, total):
    out = np.empty(total, np.uint8)
    assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), total) == 0
    return out


def random_clip(depth, n, w, h, seed):
    """Frames for the out converters: uint8 [n, h, w, 4], or float32 with values on both sides of 0 .. 1 and a NaN."""
    rng = np.random.default_rng(seed)
    if depth == 8:
        return rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    clip = (rng.random((n, h, w, 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    clip[0, 0, 0, 1] = np.nan
    return clip


def random_payloads(depth, n, w, h, seed):
    """Payloads for the in converters, every sample value allowed: out-of-range samples, the clamps and the min are exercised."""
    rng = np.random.default_rng(seed)
    samples = R8.frame_bytes(w, h)
    return rng.integers(0, 256, (n, samples), dtype=np.uint8) if depth == 8 else rng.integers(0, 1400, (n, samples)).astype(np.uint16)


def out_frames(depth, clip, mode, siting):
    """The restatement's payloads as bytes: uint8 [n, frame bytes]."""
    frames = S.frames8(clip, mode, siting) if depth == 8 else S.frames10(clip, mode, siting).astype("<u2")
    return np.ascontiguousarray(frames).view(np.uint8).reshape(len(clip), -1)


def in_frames(depth, yuv, w, h, mode, chroma, siting):
    """The restatement's destination frames as bytes: words, or float4 texels."""
    if depth == 8:
        from tests.yuv_input_reference import words
        return np.ascontiguousarray(words(S.rgba_frames(yuv, w, h, mode, chroma, siting)).astype("<u4")).view(np.uint8).reshape(len(yuv), -1)
    return np.ascontiguousarray(S.float_frames(yuv, w, h, mode, chroma, siting)).view(np.uint8).reshape(len(yuv), -1)


def in_whole(frames, dst_gap=0, dst_offset=0, mask=None):
    """The destination buffer around `frames` (bytes [n, frame]): the sentinel everywhere else, and where `mask` is False."""
    n, fb = frames.shape
    want = np.full(LEAD + dst_offset + n * (fb + dst_gap) + LEAD, SENTINEL, np.uint8)
    for i in range(n):
        at = LEAD + dst_offset + i * (fb + dst_gap)
        want[at:at + fb] = frames[i] if mask is None else np.where(mask, frames[i], SENTINEL)
    return want


def convert_out(inv, depth, clip, mode, siting="left", bands=None, offset=0, row_pad=0, frame_gap=0, dst_gap=0, dst_offset=0, sited=True, raw_siting=None):
    """Runs an out converter over clip [N, h, w, 4] -- once, or once per band into the same destination -- and returns the whole
    destination buffer.  sited=False calls the entry point without a siting; raw_siting goes to the C call as it is and
    the return code comes back with the buffer."""
    n, h, w, _ = clip.shape
    pixel = 4 if depth == 8 else 16
    stride = w * pixel + row_pad
    fstride = h * stride + frame_gap
    buf = np.full(offset + n * fstride + 16, 0x5A, np.uint8)
    rows = np.ascontiguousarray(clip).view(np.uint8).reshape(n, h, w * pixel)
    for i in range(n):
        for r in range(h):
            at = offset + i * fstride + r * stride
            buf[at:at + w * pixel] = rows[i, r]
    fb = R8.frame_bytes(w, h) * (1 if depth == 8 else 2)
    dstride = fb + dst_gap
    total = LEAD + dst_offset + n * dstride + LEAD
    src, dst = upload(buf), device_filled(total)
    call = inv.clip_to_yuv420 if depth == 8 else inv.clip_float_to_yuv420p10
    raw = lib().mmhip_clip_to_yuv420_sited if depth == 8 else lib().mmhip_clip_float_to_yuv420p10_sited
    try:
        rc = 0
        for first, last in bands or [(0, h)]:
            if raw_siting is not None:
                rc = raw(inv._h, C.c_void_p(src + offset + first * stride), stride, fstride, w, h, first, last, n, S.MATRIX_IDS[mode[0]],
                         S.RANGE_IDS[mode[1]], raw_siting, C.c_void_p(dst + LEAD + dst_offset), dstride, None)
                continue
            keywords = dict(chroma_siting=siting) if sited else {}
            call(src + offset + first * stride, dst + LEAD + dst_offset, n, width=w, height=h, rows=(first, last), src_row_stride=stride,
                 src_frame_stride=fstride, dst_frame_stride=dstride, yuv_matrix=mode[0], yuv_range=mode[1], **keywords)
        inv.sync()
        got = device_read(dst, total)
        return (rc, got) if raw_siting is not None else got
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


def convert_in(inv, depth, yuv, w, h, mode, chroma, siting="left", src_offset=0, src_gap=0, dst_gap=0, dst_offset=0, sited=True, raw_siting=None):
    """Runs an in converter over the payloads yuv [N, samples], which lie src_offset bytes into their buffer and src_gap bytes
    further apart than a frame, and returns the whole destination buffer."""
    n = len(yuv)
    payload = np.ascontiguousarray(yuv if depth == 8 else yuv.astype("<u2")).view(np.uint8).reshape(n, -1)
    fb = payload.shape[1]
    buf = np.full(src_offset + n * (fb + src_gap) + 16, 0x5A, np.uint8)
    for i in range(n):
        at = src_offset + i * (fb + src_gap)
        buf[at:at + fb] = payload[i]
    dstride = (4 if depth == 8 else 16) * w * h + dst_gap
    total = LEAD + dst_offset + n * dstride + LEAD
    src, dst = upload(buf), device_filled(total)
    call = inv.clip_from_yuv420 if depth == 8 else inv.clip_from_yuv420p10
    raw = lib().mmhip_clip_from_yuv420_sited if depth == 8 else lib().mmhip_clip_from_yuv420p10_sited
    try:
        if raw_siting is not None:
            rc = raw(inv._h, C.c_void_p(src + src_offset), fb + src_gap, w, h, n, S.MATRIX_IDS[mode[0]], S.RANGE_IDS[mode[1]], S.CHROMA_IDS[chroma],
                     raw_siting, C.c_void_p(dst + LEAD + dst_offset), dstride, None)
            inv.sync()
            return rc, device_read(dst, total)
        keywords = dict(chroma_siting=siting) if sited else {}
        call(src + src_offset, dst + LEAD + dst_offset, n, width=w, height=h, src_frame_stride=fb + src_gap, dst_frame_stride=dstride,
             yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma, **keywords)
        inv.sync()
        return device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


def launches(inv):
    """The path counters there are: (aligned, other) of the 10-bit out converter and of both in converters.  The RGBA8 out
    converter has none; its path follows from the same rule (width a multiple of 8 and everything aligned)."""
    return {("out", 10): (inv.clip_float_to_yuv420p10_launches("aligned"), inv.clip_float_to_yuv420p10_launches("bytes")),
            ("in", 8): (inv.clip_from_yuv420_launches("aligned"), inv.clip_from_yuv420_launches("bytes")),
            ("in", 10): (inv.clip_from_yuv420p10_launches("aligned"), inv.clip_from_yuv420p10_launches("samples"))}


def moved(before, after, key):
    return tuple(b - a for a, b in zip(before[key], after[key]))


# ---- 1. the four converters with left siting ----

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_out_converters_equal_the_restatement(inv, size):
    w, h = size
    for depth in DEPTHS:
        before, calls = launches(inv), 0
        for n in (1, 3):
            clip = random_clip(depth, n, w, h, 100 * w + h + n)
            for mode in MODES:
                got = convert_out(inv, depth, clip, mode)
                calls += 1
                assert np.array_equal(got, in_whole(out_frames(depth, clip, mode, "left"))), (size, depth, n, mode)
        if depth == 10:
            assert moved(before, launches(inv), ("out", 10)) == ((calls, 0) if w % 8 == 0 else (0, calls)), size
    other = random_clip(8, 1, w, h, 1)
    assert w == 1 or not np.array_equal(out_frames(8, other, mode, "left"), out_frames(8, other, mode, "center"))      # (the sitings do differ)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_in_converters_equal_the_restatement(inv, size):
    w, h = size
    for depth in DEPTHS:
        before, calls = launches(inv), 0
        for n in (1, 3):
            yuv = random_payloads(depth, n, w, h, 200 * w + h + n)
            for mode in MODES:
                for chroma in S.CHROMAS:
                    got = convert_in(inv, depth, yuv, w, h, mode, chroma)
                    calls += 1
                    assert np.array_equal(got, in_whole(in_frames(depth, yuv, w, h, mode, chroma, "left"))), (size, depth, n, mode, chroma)
        assert moved(before, launches(inv), ("in", depth)) == ((calls, 0) if w % 8 == 0 else (0, calls)), (size, depth)


# ---- 2. both paths on one source ----

@pytest.mark.parametrize("depth", DEPTHS)
def test_both_paths_give_the_same_planes(inv, depth):
    """64 x 8 out: the aligned path at an aligned pointer and with rows padded by 16, the other path a few bytes off, with rows
    padded, with frames further apart and at a destination that is off."""
    clip = random_clip(depth, 2, 64, 8, 7)
    unit = 4 if depth == 8 else 4            # source offsets stay multiples of 4 at 10 bits (floats), destinations even
    for mode in (("bt709", "limited"), ("bt601", "full")):
        frames = out_frames(depth, clip, mode, "left")
        for keywords, aligned in ((dict(), True), (dict(row_pad=16, frame_gap=32, dst_gap=16), True), (dict(offset=unit), False),
                                  (dict(row_pad=4), False), (dict(frame_gap=8, dst_gap=6), False), (dict(dst_offset=2, dst_gap=2), False)):
            before = launches(inv)
            got = convert_out(inv, depth, clip, mode, **keywords)
            want = in_whole(frames, keywords.get("dst_gap", 0), keywords.get("dst_offset", 0))
            assert np.array_equal(got, want), (depth, mode, keywords)
            if depth == 10:
                assert moved(before, launches(inv), ("out", 10)) == ((1, 0) if aligned else (0, 1)), keywords


@pytest.mark.parametrize("depth", DEPTHS)
def test_both_paths_give_the_same_frames(inv, depth):
    """64 x 8 in: base and stride off alignment, gaps on both sides."""
    w, h = 64, 8
    yuv = random_payloads(depth, 2, w, h, 11)
    step = 1 if depth == 8 else 2
    for mode in (("bt709", "limited"), ("bt601", "full")):
        frames = in_frames(depth, yuv, w, h, mode, "bilinear", "left")
        for keywords, aligned in ((dict(), True), (dict(src_gap=16, dst_gap=32), True), (dict(src_offset=step), False), (dict(src_gap=step * 2), False),
                                  (dict(src_offset=step * 3, src_gap=step * 3, dst_gap=16), False)):
            before = launches(inv)
            got = convert_in(inv, depth, yuv, w, h, mode, "bilinear", **keywords)
            assert np.array_equal(got, in_whole(frames, keywords.get("dst_gap", 0))), (depth, mode, keywords)
            assert moved(before, launches(inv), ("in", depth)) == ((1, 0) if aligned else (0, 1)), keywords


# ---- 3. rows ----

@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_bands_write_their_rows_and_nothing_else(inv, size, depth):
    w, h = size
    clip = random_clip(depth, 2, w, h, 31 + w)
    mode = ("bt709", "limited")
    frames = out_frames(depth, clip, mode, "left")
    whole = [(0, 2), (2, 6), (6, h)]
    assert np.array_equal(convert_out(inv, depth, clip, mode, bands=whole), in_whole(frames))
    for first, last in ((2, 6), (0, 2), (6, h)):
        mask = np.repeat(R8.band_mask(w, h, first, last), 1 if depth == 8 else 2)
        got = convert_out(inv, depth, clip, mode, bands=[(first, last)], dst_gap=8)
        assert np.array_equal(got, in_whole(frames, dst_gap=8, mask=mask)), (size, depth, first, last)


# ---- 4. centre through the new entry points, replicate, a siting that is neither ----

@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_centre_through_the_sited_entry_points_is_the_unsited_call(inv, size):
    w, h = size
    mode = ("bt601", "limited")
    for depth in DEPTHS:
        clip = random_clip(depth, 2, w, h, 5)
        old = convert_out(inv, depth, clip, mode, sited=False)
        assert np.array_equal(convert_out(inv, depth, clip, mode, raw_siting=0)[1], old)
        assert np.array_equal(convert_out(inv, depth, clip, mode, siting="center"), old)
        assert np.array_equal(old, in_whole(out_frames(depth, clip, mode, "center")))
        yuv = random_payloads(depth, 2, w, h, 6)
        for chroma in S.CHROMAS:
            old = convert_in(inv, depth, yuv, w, h, mode, chroma, sited=False)
            assert np.array_equal(convert_in(inv, depth, yuv, w, h, mode, chroma, raw_siting=0)[1], old)
            assert np.array_equal(convert_in(inv, depth, yuv, w, h, mode, chroma, siting="center"), old)
        # replicate ignores the siting
        assert np.array_equal(convert_in(inv, depth, yuv, w, h, mode, "replicate", raw_siting=1)[1], old)
        assert np.array_equal(convert_in(inv, depth, yuv, w, h, mode, "replicate", siting="left"), old)


def test_a_siting_that_is_neither_is_refused_and_nothing_is_written(inv):
    w, h = 17, 9
    mode = ("bt709", "limited")
    for depth, out_name, in_name in ((8, "clip_to_yuv420_sited", "clip_from_yuv420_sited"), (10, "clip_float_to_yuv420p10_sited", "clip_from_yuv420p10_sited")):
        before = launches(inv)
        rc, got = convert_out(inv, depth, random_clip(depth, 2, w, h, 1), mode, raw_siting=2)
        assert rc == -1 and err() == out_name + ": siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert (got == SENTINEL).all()
        rc, got = convert_in(inv, depth, random_payloads(depth, 2, w, h, 1), w, h, mode, "bilinear", raw_siting=2)
        assert rc == -1 and err() == in_name + ": siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
        assert (got == SENTINEL).all()
        assert launches(inv) == before
    # the host setters: refused with nothing bound
    yuv = random_payloads(8, 2, w, h, 3)
    bound = mm.Filter(PLAIN).invoke(w, h)
    bound.set_image_yuv420("in", yuv, w, h, chroma_siting="left")
    frames = bound.render_clip(num_frames=2)
    counts = launches(bound)
    assert lib().mmhip_set_image_sequence_yuv420_host_sited(bound._h, 0, yuv[::-1].copy().ctypes.data_as(C.c_void_p), yuv.shape[1], w, h, 2, 1, 0, 0, 2) == -1
    assert err() == "clip_from_yuv420_sited: siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not 2"
    assert launches(bound) == counts and np.array_equal(bound.render_clip(num_frames=2), frames)
    deep = mm.Filter(PLAIN, deep_inputs=True).invoke(w, h)
    yuv10 = random_payloads(10, 2, w, h, 3)
    deep.set_image_yuv420p10("in", yuv10, w, h, chroma_siting="left")
    frames = deep.render_clip(num_frames=2)
    counts = launches(deep)
    assert lib().mmhip_set_image_sequence_yuv420p10_host_sited(deep._h, 0, yuv10[::-1].copy().ctypes.data_as(C.c_void_p), 2 * yuv10.shape[1], w, h, 2, 1, 0,
                                                               0, -1) == -1
    assert err() == "clip_from_yuv420p10_sited: siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not -1"
    assert launches(deep) == counts and np.array_equal(deep.render_clip(num_frames=2), frames)


# ---- 5. render_clip ----

VARIANTS = {"plain": {}, "aa2": dict(aa=2), "shutter": dict(shutter_samples=3, shutter_span=0.07)}


def float_frames(inv, n, **keywords):
    """The float maps of the same call: float32 [n, h, w, 4]."""
    w, h = inv.render_width, inv.render_height
    total = n * h * w * 16
    dev = device_filled(total)
    try:
        assert inv.render_clip(out_ptr=dev, floatmap=True, **keywords) is None
        inv.sync()
        return device_read(dev, total).view(np.float32).reshape(n, h, w, 4)
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_render_clip_delivers_the_restatement_of_its_frames(variant):
    w, h, n = 17, 9, 3
    keywords = dict(num_frames=n, **VARIANTS[variant])
    inv = mm.Filter(SWIRL).invoke(w, h)
    rgba = inv.render_clip(**keywords)
    floats = float_frames(inv, n, **keywords)
    for mode in (("bt709", "limited"), ("bt601", "full")):
        names = dict(yuv_matrix=mode[0], yuv_range=mode[1])
        yuv = inv.render_clip(pixel_format="yuv420p", chroma_siting="left", **names, **keywords)
        assert yuv.dtype == np.uint8 and np.array_equal(yuv, S.frames8(rgba, mode, "left")), (variant, mode)
        deep = inv.render_clip(pixel_format="yuv420p10", chroma_siting="left", **names, **keywords)
        assert deep.dtype == np.dtype("<u2") and np.array_equal(deep, S.frames10(floats, mode, "left")), (variant, mode)
        assert not np.array_equal(yuv, S.frames8(rgba, mode, "center")) and not np.array_equal(deep, S.frames10(floats, mode, "center"))
        # centre, named or not, is the call as it was
        for siting in (dict(), dict(chroma_siting="center")):
            assert np.array_equal(inv.render_clip(pixel_format="yuv420p", **names, **siting, **keywords), R8.frames(rgba, mode))
            assert np.array_equal(inv.render_clip(pixel_format="yuv420p10", **names, **siting, **keywords), R10.frames(floats, mode))
    assert np.array_equal(inv.render_clip(**keywords), rgba)


# ---- 6. the host setters ----

@pytest.mark.parametrize("size", [(17, 9, 3), (64, 8, 2)], ids=lambda s: "%dx%dx%d" % s)
def test_a_left_sited_sequence_renders_what_the_restatements_frames_render(size):
    w, h, n = size
    for source in (PLAIN, BENT):
        for mode, chroma in ((("bt709", "limited"), "bilinear"), (("bt601", "full"), "bilinear"), (("bt709", "full"), "replicate")):
            names = dict(yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma, chroma_siting="left")
            yuv = random_payloads(8, n, w, h, 50 + w)
            inv = mm.Filter(source).invoke(w, h)
            inv.set_image_yuv420("in", yuv, w, h, **names)
            assert inv.clip_yuv_input_groups() == 1
            clip = inv.render_clip(num_frames=n)
            rgba = S.rgba_frames(yuv, w, h, mode, chroma, "left")
            inv.set_image("in", rgba)
            assert np.array_equal(clip, inv.render_clip(num_frames=n)), (source, mode, chroma)
            assert source != PLAIN or np.array_equal(clip, rgba)
            yuv10 = np.minimum(random_payloads(10, n, w, h, 60 + w), 1023)
            deep = mm.Filter(source, deep_inputs=True, intersample=source != PLAIN).invoke(w, h)      # (plain fetches the nearest texel: an identity)
            deep.set_image_yuv420p10("in", yuv10, w, h, **names)
            assert deep.clip_yuv10_input_groups() == 1
            maps = float_frames(deep, n, num_frames=n)
            texels = S.float_frames(yuv10, w, h, mode, chroma, "left")
            deep.set_image("in", texels)
            assert np.array_equal(maps.view(np.uint32), float_frames(deep, n, num_frames=n).view(np.uint32)), (source, mode, chroma)
            assert source != PLAIN or np.array_equal(maps.view(np.uint32), texels.view(np.uint32))


CHILD = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
import mathmap_amd as mm
from tests import test_gpu_clip_yuv_sited as T
inv = mm.Filter(T.BENT).invoke(17, 9)
inv.enable_timing()
inv.set_image_yuv420("in", T.random_payloads(8, 5, 17, 9, 67), 17, 9, chroma_siting="left")
labels = [name for name, ms in inv.drain_native_kernel_ms()]
out = inv.render_clip(num_frames=5)
deep = mm.Filter(T.BENT, deep_inputs=True).invoke(17, 9)
deep.enable_timing()
deep.set_image_yuv420p10("in", T.random_payloads(10, 5, 17, 9, 68), 17, 9, chroma_siting="left")
labels += [name for name, ms in deep.drain_native_kernel_ms()]
maps = T.float_frames(deep, 5, num_frames=5)
print(json.dumps({"groups": [inv.clip_yuv_input_groups(), deep.clip_yuv10_input_groups()], "labels": labels,
                  "sha": [hashlib.sha256(out.tobytes()).hexdigest(), hashlib.sha256(maps.tobytes()).hexdigest()]}))
"""


def test_groups_leave_the_frames_alone():
    """MMHIP_CLIP_YUV_IN_BYTES holds two 17 x 9 payloads of 16-bit samples (and four of bytes): 5 frames go up in 3 groups at
    10 bits and in 2 at 8 (the budget is read per call, in a child)."""
    env = dict(os.environ, MMHIP_CLIP_YUV_IN_BYTES=str(2 * R10.frame_bytes(17, 9) + 100))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["groups"] == [2, 3] and res["labels"].count("yuv420_to_rgba_clip") == 2 and res["labels"].count("yuv420p10_to_float_clip") == 3
    inv = mm.Filter(BENT).invoke(17, 9)
    inv.set_image("in", S.rgba_frames(random_payloads(8, 5, 17, 9, 67), 17, 9, ("bt709", "limited"), "bilinear", "left"))
    assert res["sha"][0] == hashlib.sha256(inv.render_clip(num_frames=5).tobytes()).hexdigest()
    deep = mm.Filter(BENT, deep_inputs=True).invoke(17, 9)
    deep.set_image("in", S.float_frames(random_payloads(10, 5, 17, 9, 68), 17, 9, ("bt709", "limited"), "bilinear", "left"))
    assert res["sha"][1] == hashlib.sha256(float_frames(deep, 5, num_frames=5).tobytes()).hexdigest()


def test_a_filter_without_deep_inputs_is_refused_and_nothing_gets_bound():
    w, h = 17, 9
    yuv = np.minimum(random_payloads(10, 2, w, h, 4), 1023)
    inv = mm.Filter(PLAIN).invoke(w, h)
    rgba = S.rgba_frames(random_payloads(8, 2, w, h, 1), w, h, ("bt709", "limited"), "bilinear", "left")
    inv.set_image("in", rgba)
    before = launches(inv)
    with pytest.raises(mm.MathMapError, match="set_image_sequence_yuv420p10_host_sited: filter `plain' was not compiled with deep_inputs"):
        inv.set_image_yuv420p10("in", yuv, w, h, chroma_siting="left")
    assert launches(inv) == before and np.array_equal(inv.render_clip(num_frames=2), rgba)


# ---- 7. the command line ----

def test_cli_writes_and_reads_left_sited_streams(tmp_path):
    def run(*args, stdin=None):
        p = subprocess.run([CLI] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout
    w, h, n = 17, 9, 3
    # out: a file and a pipe, tag and bytes of the Python path
    out = str(tmp_path / "out.y4m")
    run("-F", str(n), "-s", "%dx%d" % (w, h), "--chroma-siting=left", SWIRL, out)
    data = open(out, "rb").read()
    inv = mm.Filter(SWIRL).invoke(w, h)
    frames = inv.render_clip(num_frames=n, pixel_format="yuv420p", chroma_siting="left")
    want = io_bytes(frames, w, h, chroma_siting="left")
    assert data.startswith(b"YUV4MPEG2 W17 H9 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n") and data == want
    assert np.array_equal(frames, S.frames8(inv.render_clip(num_frames=n), ("bt709", "limited"), "left"))
    assert run("-F", str(n), "--batch-frames=2", "-s", "%dx%d" % (w, h), "--chroma-siting=left", SWIRL, "-") == data
    assert mm.api.y4m_chroma_siting(out) == "left"
    # the same options without it, or with center, give the stream as it was
    plain = run("-F", str(n), "-s", "%dx%d" % (w, h), SWIRL, "-")
    assert plain == run("-F", str(n), "-s", "%dx%d" % (w, h), "--chroma-siting=center", SWIRL, "-") == \
        R8.y4m_file(R8.frames(inv.render_clip(num_frames=n), ("bt709", "limited")), w, h)
    deep = run("-F", str(n), "-s", "%dx%d" % (w, h), "--pixel-format=yuv420p10", "--chroma-siting=left", SWIRL, "-")
    assert deep == io_bytes(inv.render_clip(num_frames=n, pixel_format="yuv420p10", chroma_siting="left"), w, h, chroma_siting="left")
    assert deep.startswith(b"YUV4MPEG2 W17 H9 F25:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n")
    # in: auto on a C420mpeg2 file is left; no option is today's bytes
    yuv = random_payloads(8, n, w, h, 77)
    src = str(tmp_path / "in.y4m")
    mm.api.write_y4m(src, yuv, w, h, chroma_siting="left")
    mode = ("bt709", "limited")
    left = R8.y4m_file(R8.frames(S.rgba_frames(yuv, w, h, mode, "bilinear", "left"), mode), w, h)
    centre = R8.y4m_file(R8.frames(S.rgba_frames(yuv, w, h, mode, "bilinear", "center"), mode), w, h)
    assert left != centre
    assert run("-Din=" + src, "--input-chroma-siting=auto", PLAIN, "-") == left
    assert run("-Din=" + src, "--input-chroma-siting=left", PLAIN, "-") == left
    assert run("-Din=-", "--input-chroma-siting=auto", PLAIN, "-", stdin=open(src, "rb").read()) == left
    assert run("-Din=" + src, PLAIN, "-") == centre == run("-Din=" + src, "--input-chroma-siting=center", PLAIN, "-")
    assert run("-Din=" + src, "--input-chroma-siting=left", "--input-chroma=replicate", PLAIN, "-") == \
        R8.y4m_file(R8.frames(S.rgba_frames(yuv, w, h, mode, "replicate", "center"), mode), w, h)
    # auto on a stream that does not say mpeg2 is centre; a 10-bit stream with left
    jpeg = str(tmp_path / "jpeg.y4m")
    mm.api.write_y4m(jpeg, yuv, w, h)
    assert run("-Din=" + jpeg, "--input-chroma-siting=auto", PLAIN, "-") == centre
    yuv10 = np.minimum(random_payloads(10, n, w, h, 78), 1023)
    src10 = str(tmp_path / "in10.y4m")
    mm.api.write_y4m(src10, yuv10, w, h)
    got = run("-Din=" + src10, "--input-chroma-siting=left", "--pixel-format=yuv420p10", PLAIN, "-")
    assert got == R10.y4m_file(R10.frames(S.float_frames(yuv10, w, h, mode, "bilinear", "left"), mode), w, h)


def io_bytes(frames, w, h, **keywords):
    import io
    data = io.BytesIO()
    mm.api.write_y4m(data, frames, w, h, **keywords)
    return data.getvalue()
