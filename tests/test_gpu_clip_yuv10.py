"""Clips as 10-bit planar Y'CbCr 4:2:0 on the GPU (mmhip_clip_float_to_yuv420p10: k_float_to_yuv420p10_clip on float
frames that stay in HBM).

The yardstick is tests/yuv10_reference.py.  Everything is compared bit for bit in whole sentinel-filled destination
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
from tests import yuv10_reference as X
from tests import yuv_reference as X8
from tests.test_gpu_clip_sampled import PROBES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
SENTINEL = 0xA5
LEAD = 64                    # sentinel bytes in front of the first and behind the last frame (keeps the base 16-byte aligned)
SWIRL = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"
# a horizontal grey ramp of 2/255 of the range around 0.401 (x runs over -X .. X): see test_the_ramp_keeps_its_steps
RAMP = "filter ramp () v = 0.401 + x / X / 255; rgba:[v, v, v, 1] end"


def err():
    return lib().mmhip_last_error().decode()


@pytest.fixture(scope="module")
def inv():
    """Any invocation: the converter uses its stream, its timing records and its counters, nothing else."""
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


def launches(inv):
    return inv.clip_float_to_yuv420p10_launches("aligned"), inv.clip_float_to_yuv420p10_launches("bytes")


def source_buffer(clip, offset=0, row_pad=0, frame_gap=0):
    """The bytes of a source buffer holding clip float32 [N, h, w, 4] `offset` bytes in, rows padded by row_pad and frames
    by frame_gap bytes (the padding holds 0x5A); returns (bytes, row_stride, frame_stride)."""
    n, h, w, _ = clip.shape
    stride = w * 16 + row_pad
    fstride = h * stride + frame_gap
    buf = np.full(offset + n * fstride + 16, 0x5A, np.uint8)
    raw = np.ascontiguousarray(clip, np.float32).view(np.uint8).reshape(n, h, w * 16)
    for i in range(n):
        for r in range(h):
            at = offset + i * fstride + r * stride
            buf[at:at + w * 16] = raw[i, r]
    return buf, stride, fstride


def convert(inv, clip, mode, bands=None, offset=0, row_pad=0, frame_gap=0, dst_gap=0, dst_offset=0):
    """Runs the converter over clip [N, h, w, 4] -- once, or once per band of `bands` into the same destination -- and
    returns the whole destination buffer: LEAD + dst_offset sentinel bytes, the frames dst_gap bytes apart, LEAD more."""
    n, h, w, _ = clip.shape
    buf, stride, fstride = source_buffer(clip, offset, row_pad, frame_gap)
    dstride = X.frame_bytes(w, h) + dst_gap
    total = LEAD + dst_offset + n * dstride + LEAD
    src, dst = upload(buf), device_filled(total)
    try:
        for first, last in bands or [(0, h)]:
            rc = lib().mmhip_clip_float_to_yuv420p10(inv._h, C.c_void_p(src + offset + first * stride), stride, fstride, w, h, first, last, n,
                                                     X.MATRIX_IDS[mode[0]], X.RANGE_IDS[mode[1]], C.c_void_p(dst + LEAD + dst_offset), dstride, None)
            assert rc == 0, err()
        inv.sync()
        return device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


def expected(clip, mode, dst_gap=0, dst_offset=0, mask=None):
    """The destination buffer convert() must return; `mask` (bool [frame_samples]): only those samples of every frame are
    written."""
    n, h, w, _ = clip.shape
    fb = X.frame_bytes(w, h)
    want = np.full(LEAD + dst_offset + n * (fb + dst_gap) + LEAD, SENTINEL, np.uint8)
    for i in range(n):
        at = LEAD + dst_offset + i * (fb + dst_gap)
        frame = X.frame(clip[i], mode).astype("<u2")
        if mask is not None:
            frame = np.where(mask, frame, SENTINEL * 257).astype("<u2")
        want[at:at + fb] = frame.view(np.uint8)
    return want


def random_clip(n, w, h, seed):
    """Floats of which a part lies in 0 .. 1 and a part outside, with NaN, both infinities and -0 planted, and with
    values on and beside the quantiser's ties (k + 0.5) / 65535."""
    rng = np.random.default_rng(seed)
    clip = rng.uniform(-0.25, 1.25, (n, h, w, 4)).astype(np.float32)
    flat = clip.reshape(-1)
    some = rng.permutation(flat.size)
    k = max(flat.size // 8, 1)
    ties = ((rng.integers(0, 65535, k) + 0.5) / 65535.0).astype(np.float32)
    step = rng.integers(-1, 2, k)
    ties = np.where(step > 0, np.nextafter(ties, np.float32(2)), np.where(step < 0, np.nextafter(ties, np.float32(-1)), ties))
    flat[some[:k]] = ties
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.5, np.finfo(np.float32).smallest_subnormal], np.float32)
    m = min(len(specials), max(flat.size - k, 0))
    flat[some[k:k + m]] = specials[:m]
    return clip


# ---- 1. the converter alone ----

SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (5, 3), (7, 7), (8, 2), (16, 2), (17, 9), (24, 4), (64, 8), (63, 8), (72, 6), (256, 2), (9, 17)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_converter_equals_the_restatement(inv, size):
    w, h = size
    before = launches(inv)
    for n in (1, 3):
        clip = random_clip(n, w, h, 100 * w + h + n)
        for mode in X.MODES:
            got = convert(inv, clip, mode)
            assert np.array_equal(got, expected(clip, mode)), (size, n, mode)
    after = launches(inv)
    aligned = w % 8 == 0                # (the buffers of convert() are 16-byte aligned and packed)
    assert (after[0] - before[0], after[1] - before[1]) == ((8, 0) if aligned else (0, 8))
    # alpha does not matter
    other = clip.copy()
    other[..., 3] = np.where(np.isfinite(other[..., 3]), 1 - other[..., 3], 0.25)
    assert np.array_equal(convert(inv, other, X.MODES[0]), convert(inv, clip, X.MODES[0]))


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_both_paths_give_the_same_planes(inv, mode):
    """64 x 8: the path of wide accesses at an aligned pointer, with rows padded by 16 and frames 32 bytes further apart;
    the path of per-pixel accesses at a base 4 bytes off, with rows padded by 4, with frames 8 bytes further apart and at a
    destination 2, 4 or 8 bytes off or with frames 2 bytes further apart.  The launcher's choice is read from the counters."""
    clip = random_clip(2, 64, 8, 7)
    want = expected(clip, mode)

    def path_of(**case):
        before = launches(inv)
        got = convert(inv, clip, mode, **case)
        after = launches(inv)
        assert np.array_equal(got, expected(clip, mode, dst_gap=case.get("dst_gap", 0), dst_offset=case.get("dst_offset", 0))), case
        return {(1, 0): "aligned", (0, 1): "bytes"}[(after[0] - before[0], after[1] - before[1])]
    assert np.array_equal(convert(inv, clip, mode), want)
    for case in (dict(), dict(row_pad=16), dict(offset=16), dict(frame_gap=32), dict(dst_offset=16), dict(dst_gap=16)):
        assert path_of(**case) == "aligned", case
    for case in (dict(offset=4), dict(row_pad=4), dict(frame_gap=8), dict(offset=8, row_pad=12), dict(dst_offset=2), dict(dst_offset=4), dict(dst_offset=8),
                 dict(dst_gap=2), dict(dst_gap=8)):
        assert path_of(**case) == "bytes", case


# ---- 2. every channel value ----

def walk_frame():
    """256 x 256: pixel p = 256 y + x has the channels (p, 7 p + 3, 65535 - p) / 65535 mod 2^16 -- every one of the 2^16
    values in every channel, in orders that differ."""
    p = np.arange(1 << 16, dtype=np.int64)
    q = np.stack([p, (7 * p + 3) % 65536, 65535 - p, (p * 31) % 65536], axis=1)
    clip = (q / 65535.0).astype(np.float32).reshape(1, 256, 256, 4)
    return clip, q


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_every_channel_value(inv, mode):
    clip, q = walk_frame()
    assert all(len(np.unique(X.quant(clip[..., c]))) == 65536 for c in range(3))
    got = convert(inv, clip, mode)
    assert np.array_equal(got, expected(clip, mode))


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_blocks_of_corner_colours(inv, mode):
    """128 x 128: the 8^4 blocks of four corner colours, pure blue and pure red at full range (1023.5 in the real formula)
    among them."""
    corners = np.array([(r, g, b, 0) for r in (0, 1) for g in (0, 1) for b in (0, 1)], np.float32)
    k = np.arange(4096).reshape(64, 64)
    clip = np.empty((1, 128, 128, 4), np.float32)
    for j in (0, 1):
        for i in (0, 1):
            clip[0, j::2, i::2] = corners[(k >> (3 * (2 * j + i))) & 7]
    got = convert(inv, clip, mode)
    assert np.array_equal(got, expected(clip, mode))
    y, cb, cr = mm.api.yuv420_planes(got[LEAD:LEAD + X.frame_bytes(128, 128)].view("<u2"), 128, 128)
    blue, red = 1, 4                  # index k of a block of one colour: the colour's index in all four places
    at = lambda c: divmod(c * (1 + 8 + 64 + 512), 64)
    if mode[1] == "full":
        assert cb[0][at(blue)] == 1023 and cr[0][at(red)] == 1023 and cb.max() == 1023 and cr.max() == 1023 and y.max() == 1023 and y.min() == 0
    else:
        assert cb[0][at(blue)] == 960 and cr[0][at(red)] == 960 and cb.min() == 64 and cr.min() == 64 and cb.max() == 960 and cr.max() == 960
        assert y.max() == 940 and y.min() == 64


# ---- 3. bands, strides, refusals ----

@pytest.mark.parametrize("case", ["17x9", "64x8"])
def test_bands_equal_the_whole_frame_call(inv, case):
    (w, h), bands = {"17x9": ((17, 9), [(0, 2), (2, 8), (8, 9)]), "64x8": ((64, 8), [(0, 4), (4, 8)])}[case]
    clip = random_clip(3, w, h, 21)
    mode = ("bt709", "limited")
    whole = convert(inv, clip, mode)
    assert np.array_equal(whole, expected(clip, mode))
    assert np.array_equal(convert(inv, clip, mode, bands=bands), whole)
    assert np.array_equal(convert(inv, clip, mode, bands=bands[::-1], dst_gap=6), expected(clip, mode, dst_gap=6))
    masks = [X.band_mask(w, h, *band) for band in bands]
    assert (sum(m.astype(int) for m in masks) == 1).all()                  # the bands' samples are disjoint and cover the frame
    for band, mask in zip(bands, masks):
        assert np.array_equal(convert(inv, clip, mode, bands=[band]), expected(clip, mode, mask=mask)), band


def test_calls_that_break_a_rule_are_refused_by_name_and_write_nothing(inv):
    fb = X.frame_bytes(17, 9)
    src, dst = upload(random_clip(1, 17, 9, 5)), device_filled(fb + 2)
    try:
        def call(first, last, dstride=fb, matrix=1, rng=0, n=1, stride=272, src_off=0, dst_off=0):
            return lib().mmhip_clip_float_to_yuv420p10(inv._h, C.c_void_p(src + src_off), stride, stride * 9, 17, 9, first, last, n, matrix, rng,
                                                       C.c_void_p(dst + dst_off), dstride, None)
        before = launches(inv)
        assert call(1, 4) == -1 and err() == "clip_float_to_yuv420p10: first_row must be even, not 1"
        assert call(3, 9) == -1 and "first_row must be even" in err()
        assert call(0, 3) == -1 and err() == "clip_float_to_yuv420p10: last_row must be even or equal to height, not 3 of 9"
        assert call(2, 7) == -1 and "last_row must be even or equal to height" in err()
        assert call(0, 9, dstride=fb - 2) == -1 and err() == "clip_float_to_yuv420p10: dst_frame_stride 484 is smaller than one frame (486 bytes)"
        assert call(0, 9, dstride=fb + 1) == -1 and "must be even" in err()
        assert call(0, 9, dst_off=1) == -1 and "must be even" in err()
        assert call(0, 9, src_off=2) == -1 and "multiples of 4" in err()
        assert call(0, 9, stride=270) == -1 and "smaller than one row (272 bytes)" in err()
        assert call(0, 9, matrix=2) == -1 and "matrix must be" in err()
        assert call(0, 9, rng=-1) == -1 and "range must be" in err()
        assert call(0, 9, n=65536) == -1 and "more than 65535 frames" in err()
        assert call(0, 9, n=0) == -1 and "num_frames must be at least 1" in err()
        inv.sync()
        assert (device_read(dst, fb + 2) == SENTINEL).all() and launches(inv) == before
        assert call(8, 9) == 0 and call(0, 8) == 0
    finally:
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_larger_strides_on_both_sides_leave_the_gaps_alone(inv, size):
    clip = random_clip(3, size[0], size[1], 33)
    for gap, row_pad, frame_gap in ((2, 16, 0), (16, 0, 64), (24, 32, 16), (1000, 4, 4)):
        for mode in (("bt601", "full"), ("bt709", "limited")):
            got = convert(inv, clip, mode, dst_gap=gap, row_pad=row_pad, frame_gap=frame_gap)
            assert np.array_equal(got, expected(clip, mode, dst_gap=gap)), (gap, row_pad, frame_gap, mode)


# ---- 4. through render_clip ----

NAMES = ["rotate", "pair", "wave", "blur"]
VARIANTS = {
    "plain": {},
    "shutter": dict(shutter_samples=3, shutter_span=0.07),
    "aa2": dict(aa=2),
    "aa2-tent": dict(aa=2, aa_filter="tent"),
    "aa4-adaptive": dict(aa=4, aa_threshold=0.05),
}
FRAMES, TS = [2, 0, 1], [0.9, 0.1, 0.5]
_filters = {}


def probe(name, w, h):
    from tests import filters as F
    if name not in _filters:
        src, opts, image, _ = PROBES[name]
        _filters[name] = (mm.Filter(src, **opts), image)
    flt, image = _filters[name]
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        inv.set_image("in", F.synthetic_image(w, h, seed=5) if image is None else image)
    return inv


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
@pytest.mark.parametrize("name", NAMES)
def test_render_clip_delivers_the_restatement_of_its_float_frames(name, variant):
    keywords = VARIANTS[variant]
    modes = {(17, 9): ("bt709", "limited"), (64, 8): ("bt601", "full")}
    for (w, h), mode in modes.items():
        inv = probe(name, w, h)
        rgba = inv.render_clip(frames=FRAMES, ts=TS, **keywords)
        yuv8 = inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p", yuv_matrix=mode[0], yuv_range=mode[1], **keywords)
        assert np.array_equal(yuv8, X8.frames(rgba, mode))
        floats = float_frames(inv, 3, frames=FRAMES, ts=TS, **keywords)
        default = mode == ("bt709", "limited")
        yuv = inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p10", **keywords) if default else \
            inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p10", yuv_matrix=mode[0], yuv_range=mode[1], **keywords)
        assert yuv.dtype == np.dtype("<u2") and yuv.shape == (3, X.frame_samples(w, h))
        assert np.array_equal(yuv, X.frames(floats, mode)), (name, variant, w, h)
        assert yuv.max() <= 1023
        # the calls around it give their earlier bytes
        assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, **keywords), rgba)
        assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p", yuv_matrix=mode[0], yuv_range=mode[1], **keywords), yuv8)
    assert len({X.frames(floats, m).tobytes() for m in X.MODES}) == 4                                # (the modes do differ on these frames)


def test_render_clip_into_device_memory_whole_and_in_bands():
    w, h = 17, 9
    inv = probe("rotate", w, h)
    mode = ("bt709", "limited")
    floats = float_frames(inv, 3, num_frames=3, shutter_samples=2, shutter=0.5)
    fb = X.frame_bytes(w, h)
    assert fb == mm.api.yuv420_frame_bytes(w, h, "yuv420p10")
    want = np.full(LEAD + 3 * fb + LEAD, SENTINEL, np.uint8)
    want[LEAD:LEAD + 3 * fb] = X.frames(floats, mode).astype("<u2").view(np.uint8).reshape(-1)
    for bands in ([None], [(0, 2), (2, 8), (8, 9)]):
        dev = device_filled(len(want))
        try:
            for rows in bands:
                assert inv.render_clip(num_frames=3, shutter_samples=2, shutter=0.5, out_ptr=dev + LEAD, rows=rows, pixel_format="yuv420p10") is None
            inv.sync()
            assert np.array_equal(device_read(dev, len(want)), want), bands
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
    # the raw call on frames this process rendered itself
    src, dst = upload(floats), device_filled(len(want))
    try:
        inv.clip_float_to_yuv420p10(src, dst + LEAD, 3)
        inv.sync()
        assert np.array_equal(device_read(dst, len(want)), want)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    with pytest.raises(ValueError, match="rows"):
        inv.render_clip(num_frames=3, out_ptr=1 << 20, rows=(1, 4), pixel_format="yuv420p10")
    with pytest.raises(mm.api.MathMapError, match="out_ptr"):
        inv.render_clip(num_frames=3, rows=(0, 4), pixel_format="yuv420p10")


CHILD = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_clip_yuv10 import probe
inv = probe("rotate", 17, 9)
inv.enable_timing()
out = inv.render_clip(num_frames=5, shutter_samples=2, shutter=0.5, pixel_format="yuv420p10")
print(json.dumps({"labels": [name for name, ms in inv.drain_native_kernel_ms()], "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


def test_groups_leave_the_samples_alone_and_are_timed_once_each():
    """MMHIP_CLIP_YUV_BYTES holds two 17 x 9 float frames: 5 frames take 3 groups (the budget is read per call, in a child)."""
    env = dict(os.environ, MMHIP_CLIP_YUV_BYTES=str(2 * 17 * 9 * 16 + 100))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["labels"].count("yuv420p10_clip") == 3 and res["labels"].count("yuv420_clip") == 0
    inv = probe("rotate", 17, 9)
    inv.enable_timing()
    inv.drain_native_kernel_ms()
    single = inv.render_clip(num_frames=5, shutter_samples=2, shutter=0.5, pixel_format="yuv420p10")
    assert [name for name, ms in inv.drain_native_kernel_ms()].count("yuv420p10_clip") == 1
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()
    floats = float_frames(inv, 5, num_frames=5, shutter_samples=2, shutter=0.5)
    assert np.array_equal(single, X.frames(floats, ("bt709", "limited")))


# ---- 5. the point of it ----

@pytest.mark.parametrize("mode", [("bt709", "limited"), ("bt709", "full")], ids="-".join)
def test_the_ramp_keeps_its_steps(mode):
    """A horizontal grey ramp over 64 columns that spans 2/255 of the range: two 8-bit steps, so the RGBA8 frame holds at
    most 3 levels and so does its Y plane; at 10 bits the span is 2/255 * 876 = 6.9 codes (8.0 at full range), of which the
    pixel centres cover 63/64: with the ramp placed at 0.401 that is at least 8 distinct codes.  Both counts are taken from
    the restatements on the CPU first, then from the GPU's planes, which must equal them."""
    w, h = 64, 8
    inv = mm.Filter(RAMP).invoke(w, h)
    floats = float_frames(inv, 1, num_frames=1)
    v = floats[0, 0, :, 0]
    assert (np.diff(v) > 0).all() and 1.9 / 255 * 63 / 64 < float(v[-1]) - float(v[0]) < 2.0 / 255
    rgba = inv.render_clip(num_frames=1)
    want10, want8 = X.frames(floats, mode), X8.frames(rgba, mode)
    steps10 = len(np.unique(mm.api.yuv420_planes(want10, w, h)[0]))
    steps8 = len(np.unique(mm.api.yuv420_planes(want8, w, h)[0]))
    print("distinct Y codes over the ramp, %s %s: %d at 10 bits, %d at 8 bits" % (mode + (steps10, steps8)))
    assert steps10 >= 8 and steps8 <= 3
    got10 = inv.render_clip(num_frames=1, pixel_format="yuv420p10", yuv_matrix=mode[0], yuv_range=mode[1])
    got8 = inv.render_clip(num_frames=1, pixel_format="yuv420p", yuv_matrix=mode[0], yuv_range=mode[1])
    assert np.array_equal(got10, want10) and np.array_equal(got8, want8)
    y10, cb10, cr10 = mm.api.yuv420_planes(got10, w, h)
    assert len(np.unique(y10)) >= 8 and len(np.unique(mm.api.yuv420_planes(got8, w, h)[0])) <= 3
    assert (cb10 == 512).all() and (cr10 == 512).all() and (np.diff(y10[0, 0].astype(int)) >= 0).all()


# ---- 6. the command line ----

def test_cli_writes_one_10_bit_y4m_file(tmp_path):
    def run(*args, ok=True):
        p = subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout if ok else p.stderr.decode()
    out = str(tmp_path / "out.y4m")
    run("-F", "3", "-s", "17x9", "--pixel-format=yuv420p10", SWIRL, out)
    data = open(out, "rb").read()
    inv = mm.Filter(SWIRL).invoke(17, 9)
    want = X.frames(float_frames(inv, 3, num_frames=3), ("bt709", "limited"))
    assert data.startswith(b"YUV4MPEG2 W17 H9 F25:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n")
    fields, frames = X.parse_y4m(data)
    assert fields == {"W": "17", "H": "9", "F": "25:1", "I": "p", "A": "1:1", "C": "420p10", "XCOLORRANGE": "LIMITED"}
    assert np.array_equal(frames, want)
    assert data == X.y4m_file(frames, 17, 9)
    assert [p.name for p in tmp_path.iterdir()] == ["out.y4m"]
    # the same stream on standard output, in batches of two frames
    assert run("-F", "3", "--batch-frames=2", "-s", "17x9", "--pixel-format=yuv420p10", SWIRL, "-") == data
    # the other mode, a frame rate, an anti-aliased clip
    out = str(tmp_path / "full.y4m")
    run("-F", "3", "-s", "64x8", "--aa=2", "--yuv-matrix=bt601", "--yuv-range=full", "--fps=30000:1001", "--pixel-format=yuv420p10", SWIRL, out)
    data = open(out, "rb").read()
    want = X.frames(float_frames(mm.Filter(SWIRL).invoke(64, 8), 3, num_frames=3, aa=2), ("bt601", "full"))
    assert data.startswith(b"YUV4MPEG2 W64 H8 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n")
    fields, frames = X.parse_y4m(data)
    assert np.array_equal(frames, want)
    assert data == X.y4m_file(frames, 64, 8, (30000, 1001), "full")
    # -F 1 (and no -F at all) gives a one-frame file
    for extra in (["-F", "1"], []):
        out = str(tmp_path / "one.y4m")
        run(*extra, "-s", "17x9", "--pixel-format=yuv420p10", SWIRL, out)
        fields, frames = X.parse_y4m(open(out, "rb").read())
        assert frames.shape == (1, X.frame_samples(17, 9))
        assert np.array_equal(frames, X.frames(float_frames(inv, 1, num_frames=1), ("bt709", "limited")))
    # --pixel-format=yuv420p is the 8-bit file as it was
    out8, plain8 = str(tmp_path / "p8.y4m"), str(tmp_path / "plain8.y4m")
    run("-F", "3", "-s", "17x9", "--pixel-format=yuv420p", SWIRL, out8)
    run("-F", "3", "-s", "17x9", SWIRL, plain8)
    assert open(out8, "rb").read() == open(plain8, "rb").read()
    # refused with -o
    before = sorted(p.name for p in tmp_path.iterdir())
    assert "not combined with -o" in run("-o", "-F", "3", "-s", "17x9", "--pixel-format=yuv420p10", SWIRL, str(tmp_path / "o.y4m"), ok=False)
    assert sorted(p.name for p in tmp_path.iterdir()) == before
