"""Clips as planar Y'CbCr 4:2:0 on the GPU (mmhip_clip_to_yuv420: k_rgba8_to_yuv420_clip on frames that stay in HBM).

The yardstick is tests/yuv_reference.py.  Everything is compared byte for byte in whole sentinel-filled destination
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
from tests import yuv_reference as X
from tests.test_gpu_clip_sampled import PROBES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
SENTINEL = 0xA5
LEAD = 64                    # sentinel bytes in front of the first and behind the last frame (keeps the base 16-byte aligned)
SWIRL = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a * 5 + t * 3), frame / 6, 1] end"


def err():
    return lib().mmhip_last_error().decode()


@pytest.fixture(scope="module")
def inv():
    """Any invocation: the converter uses its stream and its timing records, nothing else."""
    return mm.Filter("filter f () rgba:[t, 0, 0, 1] end").invoke(8, 8)


def device_filled(total):
    p = lib().mmhip_device_alloc(total)
    assert p
    fill = np.full(total, SENTINEL, np.uint8)
    assert lib().mmhip_copy_to_device(C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), total) == 0
    return p


def upload(array):
    array = np.ascontiguousarray(array, np.uint8)
    p = lib().mmhip_device_alloc(array.nbytes)
    assert p
    assert lib().mmhip_copy_to_device(C.c_void_p(p), array.ctypes.data_as(C.c_void_p), array.nbytes) == 0
    return p


def device_read(p, total):
    out = np.empty(total, np.uint8)
    assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), total) == 0
    return out


def source_buffer(clip, offset=0, row_pad=0, frame_gap=0):
    """The bytes of a source buffer holding clip [N, h, w, 4] `offset` bytes in, rows padded by row_pad and frames by
    frame_gap bytes (the padding holds 0x5A); returns (bytes, row_stride, frame_stride)."""
    n, h, w, _ = clip.shape
    stride = w * 4 + row_pad
    fstride = h * stride + frame_gap
    buf = np.full(offset + n * fstride + 16, 0x5A, np.uint8)
    for i in range(n):
        for r in range(h):
            at = offset + i * fstride + r * stride
            buf[at:at + w * 4] = clip[i, r].reshape(-1)
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
            rc = lib().mmhip_clip_to_yuv420(inv._h, C.c_void_p(src + offset + first * stride), stride, fstride, w, h, first, last, n,
                                            X.MATRIX_IDS[mode[0]], X.RANGE_IDS[mode[1]], C.c_void_p(dst + LEAD + dst_offset), dstride, None)
            assert rc == 0, err()
        inv.sync()
        return device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


def expected(clip, mode, dst_gap=0, dst_offset=0, mask=None):
    """The destination buffer convert() must return; `mask` (bool [frame_bytes]): only those bytes of every frame are written."""
    n, h, w, _ = clip.shape
    fb = X.frame_bytes(w, h)
    want = np.full(LEAD + dst_offset + n * (fb + dst_gap) + LEAD, SENTINEL, np.uint8)
    for i in range(n):
        at = LEAD + dst_offset + i * (fb + dst_gap)
        frame = X.frame(clip[i], mode)
        if mask is not None:
            frame = np.where(mask, frame, SENTINEL).astype(np.uint8)
        want[at:at + fb] = frame
    return want


def random_clip(n, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), dtype=np.uint8)


# ---- 1. the converter alone ----

SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (7, 3), (8, 2), (16, 2), (24, 4), (9, 2), (15, 6), (17, 9), (31, 33), (64, 8), (65, 7), (97, 61)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_converter_equals_the_restatement(inv, size):
    w, h = size
    for n in (1, 3):
        clip = random_clip(n, w, h, 100 * w + h + n)
        for mode in X.MODES:
            got = convert(inv, clip, mode)
            assert np.array_equal(got, expected(clip, mode)), (size, n, mode)
    # the alpha byte does not matter
    other = clip.copy()
    other[..., 3] = 255 - other[..., 3]
    assert np.array_equal(convert(inv, other, X.MODES[0]), convert(inv, clip, X.MODES[0]))


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_both_paths_give_the_same_planes(inv, mode):
    """64 x 8: the path of wide accesses at an aligned pointer and with rows padded by 16, the path of byte accesses 4
    bytes off, with rows padded by 4, with frames 8 bytes further apart and at a destination 4 bytes off."""
    clip = random_clip(2, 64, 8, 7)
    want = expected(clip, mode)
    assert np.array_equal(convert(inv, clip, mode), want)
    for case in (dict(offset=4), dict(row_pad=4), dict(row_pad=16), dict(offset=16), dict(offset=1, row_pad=3), dict(frame_gap=8), dict(frame_gap=16)):
        assert np.array_equal(convert(inv, clip, mode, **case), want), case
    for dst_offset in (4, 8, 1):
        assert np.array_equal(convert(inv, clip, mode, dst_offset=dst_offset), expected(clip, mode, dst_offset=dst_offset)), dst_offset


# ---- 2. every colour ----

@pytest.fixture(scope="module")
def every_colour():
    """4096 x 4096: pixel p = 4096 y + x is the colour R = p & 255, G = (p >> 8) & 255, B = p >> 16, under a random alpha."""
    p = np.arange(1 << 24, dtype=np.uint32)
    rgba = np.empty((1, 4096, 4096, 4), np.uint8)
    flat = rgba.reshape(-1, 4)
    flat[:, 0], flat[:, 1], flat[:, 2] = p & 255, (p >> 8) & 255, p >> 16
    flat[:, 3] = np.random.default_rng(3).integers(0, 256, 1 << 24, dtype=np.uint8)
    return rgba


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_every_colour(inv, every_colour, mode):
    w = h = 4096
    src, dst = upload(every_colour), device_filled(X.frame_bytes(w, h) + LEAD)
    try:
        assert lib().mmhip_clip_to_yuv420(inv._h, C.c_void_p(src), w * 4, w * h * 4, w, h, 0, h, 1, X.MATRIX_IDS[mode[0]], X.RANGE_IDS[mode[1]],
                                          C.c_void_p(dst), X.frame_bytes(w, h), None) == 0, err()
        inv.sync()
        got = device_read(dst, X.frame_bytes(w, h) + LEAD)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    assert (got[X.frame_bytes(w, h):] == SENTINEL).all()
    y, cb, cr = mm.api.yuv420_planes(got[:X.frame_bytes(w, h)], w, h)
    for r0 in range(0, h, 512):                         # (the restatement works in int64: a slice of rows at a time)
        assert np.array_equal(y[0, r0:r0 + 512], X.luma(every_colour[0, r0:r0 + 512, :, :3], mode).astype(np.uint8)), r0
    # chroma at 2^20 random blocks
    rng = np.random.default_rng(11)
    cx, cy = rng.integers(0, 2048, 1 << 20), rng.integers(0, 2048, 1 << 20)
    sums = sum(every_colour[0, 2 * cy + j, 2 * cx + i, :3].astype(np.int64) for j in (0, 1) for i in (0, 1))
    want_cb, want_cr = X.chroma(sums, mode)
    assert np.array_equal(cb[0, cy, cx], want_cb) and np.array_equal(cr[0, cy, cx], want_cr)


@pytest.mark.parametrize("mode", X.MODES, ids="-".join)
def test_blocks_of_corner_colours(inv, mode):
    """128 x 128: the 8^4 blocks of four corner colours, the clamp at full range among them."""
    corners = np.array([(r, g, b, 0) for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    k = np.arange(4096).reshape(64, 64)
    clip = np.empty((1, 128, 128, 4), np.uint8)
    for j in (0, 1):
        for i in (0, 1):
            clip[0, j::2, i::2] = corners[(k >> (3 * (2 * j + i))) & 7]
    got = convert(inv, clip, mode)
    assert np.array_equal(got, expected(clip, mode))
    y, cb, cr = mm.api.yuv420_planes(got[LEAD:LEAD + X.frame_bytes(128, 128)], 128, 128)
    blue, red = 1, 4                  # index k of a block of one colour: the colour's index in all four places
    at = lambda c: divmod(c * (1 + 8 + 64 + 512), 64)
    if mode[1] == "full":
        assert cb[0][at(blue)] == 255 and cr[0][at(red)] == 255
    else:
        assert cb[0][at(blue)] == 240 and cr[0][at(red)] == 240 and cb.min() == 16 and cr.min() == 16 and cb.max() == 240 and cr.max() == 240


# ---- 3. bands, strides, refusals ----

@pytest.mark.parametrize("case", ["17x9", "64x8"])
def test_bands_equal_the_whole_frame_call(inv, case):
    (w, h), bands = {"17x9": ((17, 9), [(0, 2), (2, 8), (8, 9)]), "64x8": ((64, 8), [(0, 4), (4, 8)])}[case]
    clip = random_clip(3, w, h, 21)
    mode = ("bt709", "limited")
    whole = convert(inv, clip, mode)
    assert np.array_equal(whole, expected(clip, mode))
    assert np.array_equal(convert(inv, clip, mode, bands=bands), whole)
    assert np.array_equal(convert(inv, clip, mode, bands=bands[::-1], dst_gap=5), expected(clip, mode, dst_gap=5))
    masks = [X.band_mask(w, h, *band) for band in bands]
    assert (sum(m.astype(int) for m in masks) == 1).all()                  # the bands' bytes are disjoint and cover the frame
    for band, mask in zip(bands, masks):
        assert np.array_equal(convert(inv, clip, mode, bands=[band]), expected(clip, mode, mask=mask)), band


def test_rows_that_break_the_rule_are_refused_by_name(inv):
    src, dst = upload(random_clip(1, 17, 9, 5)), device_filled(X.frame_bytes(17, 9))
    try:
        def call(first, last, dstride=X.frame_bytes(17, 9), matrix=1, rng=0, n=1):
            return lib().mmhip_clip_to_yuv420(inv._h, C.c_void_p(src), 68, 68 * 9, 17, 9, first, last, n, matrix, rng, C.c_void_p(dst), dstride, None)
        assert call(1, 4) == -1 and err() == "clip_to_yuv420: first_row must be even, not 1"
        assert call(3, 9) == -1 and "first_row must be even" in err()
        assert call(0, 3) == -1 and err() == "clip_to_yuv420: last_row must be even or equal to height, not 3 of 9"
        assert call(2, 7) == -1 and "last_row must be even or equal to height" in err()
        assert call(0, 9, dstride=X.frame_bytes(17, 9) - 1) == -1 and err() == "clip_to_yuv420: dst_frame_stride 242 is smaller than one frame (243 bytes)"
        assert call(0, 9, matrix=2) == -1 and "matrix must be" in err()
        assert call(0, 9, rng=-1) == -1 and "range must be" in err()
        assert call(0, 9, n=65536) == -1 and "more than 65535 frames" in err()
        inv.sync()
        assert (device_read(dst, X.frame_bytes(17, 9)) == SENTINEL).all()
        assert call(8, 9) == 0 and call(0, 8) == 0
    finally:
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_a_larger_frame_stride_leaves_the_gaps_alone(inv, size):
    clip = random_clip(3, size[0], size[1], 33)
    for gap in (1, 8, 24, 1000):
        for mode in (("bt601", "full"), ("bt709", "limited")):
            assert np.array_equal(convert(inv, clip, mode, dst_gap=gap), expected(clip, mode, dst_gap=gap)), (gap, mode)


# ---- 4. through render_clip ----

NAMES = ["rotate", "pair", "wave", "blur"]
VARIANTS = {
    "plain": {},
    "shutter": dict(shutter_samples=3, shutter_span=0.07),
    "aa2": dict(aa=2),
    "aa2-tent": dict(aa=2, aa_filter="tent"),
    "aa4-adaptive": dict(aa=4, aa_threshold=0.05),
    "supersample": dict(supersample=True),
}
FRAMES, TS = [2, 0, 1], [0.9, 0.1, 0.5]
_filters = {}


def probe(name, supersampling, w, h):
    from tests import filters as F
    key = (name, supersampling)
    if key not in _filters:
        src, opts, image, _ = PROBES[name]
        _filters[key] = (mm.Filter(src, supersampling=supersampling, **opts), image)
    flt, image = _filters[key]
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        inv.set_image("in", F.synthetic_image(w, h, seed=5) if image is None else image)
    return inv


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_render_clip_delivers_the_restatement_of_its_rgba_frames(name, variant):
    keywords = VARIANTS[variant]
    modes = {(17, 9): ("bt709", "limited"), (64, 8): ("bt601", "full")}
    for (w, h), mode in modes.items():
        inv = probe(name, variant == "supersample", w, h)
        rgba = inv.render_clip(frames=FRAMES, ts=TS, **keywords)
        assert rgba.shape == (3, h, w, 4)
        default = mode == ("bt709", "limited")
        yuv = inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p", **keywords) if default else \
            inv.render_clip(frames=FRAMES, ts=TS, pixel_format="yuv420p", yuv_matrix=mode[0], yuv_range=mode[1], **keywords)
        assert yuv.dtype == np.uint8 and yuv.shape == (3, X.frame_bytes(w, h))
        assert np.array_equal(yuv, X.frames(rgba, mode)), (name, variant, w, h)
        assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, **keywords), rgba)              # and the plain call is what it was
    assert len({X.frames(rgba, m).tobytes() for m in X.MODES}) == 4                                # (the modes do differ on these frames)


def test_render_clip_into_device_memory_whole_and_in_bands():
    w, h = 17, 9
    inv = probe("rotate", False, w, h)
    mode = ("bt709", "limited")
    rgba = inv.render_clip(num_frames=3, shutter_samples=2, shutter=0.5)
    fb = X.frame_bytes(w, h)
    want = np.full(LEAD + 3 * fb + LEAD, SENTINEL, np.uint8)
    want[LEAD:LEAD + 3 * fb] = X.frames(rgba, mode).reshape(-1)
    for bands in ([None], [(0, 2), (2, 8), (8, 9)]):
        dev = device_filled(len(want))
        try:
            for rows in bands:
                assert inv.render_clip(num_frames=3, shutter_samples=2, shutter=0.5, out_ptr=dev + LEAD, rows=rows, pixel_format="yuv420p") is None
            inv.sync()
            assert np.array_equal(device_read(dev, len(want)), want), bands
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
    # the raw call on frames this process rendered itself
    src, dst = upload(rgba), device_filled(len(want))
    try:
        inv.clip_to_yuv420(src, dst + LEAD, 3)
        inv.sync()
        assert np.array_equal(device_read(dst, len(want)), want)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    with pytest.raises(ValueError, match="rows"):
        inv.render_clip(num_frames=3, out_ptr=1 << 20, rows=(1, 4), pixel_format="yuv420p")
    with pytest.raises(mm.api.MathMapError, match="out_ptr"):
        inv.render_clip(num_frames=3, rows=(0, 4), pixel_format="yuv420p")


CHILD = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_clip_yuv import probe
inv = probe("rotate", False, 17, 9)
inv.enable_timing()
out = inv.render_clip(num_frames=5, shutter_samples=2, shutter=0.5, pixel_format="yuv420p")
print(json.dumps({"labels": [name for name, ms in inv.drain_native_kernel_ms()], "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


def test_groups_leave_the_bytes_alone_and_are_timed_once_each():
    """MMHIP_CLIP_YUV_BYTES holds two 17 x 9 RGBA8 frames: 5 frames take 3 groups (the budget is read per call, in a child)."""
    env = dict(os.environ, MMHIP_CLIP_YUV_BYTES=str(2 * 17 * 9 * 4 + 100))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["labels"].count("yuv420_clip") == 3
    inv = probe("rotate", False, 17, 9)
    inv.enable_timing()
    inv.drain_native_kernel_ms()
    single = inv.render_clip(num_frames=5, shutter_samples=2, shutter=0.5, pixel_format="yuv420p")
    assert [name for name, ms in inv.drain_native_kernel_ms()].count("yuv420_clip") == 1
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()
    rgba = inv.render_clip(num_frames=5, shutter_samples=2, shutter=0.5)
    assert np.array_equal(single, X.frames(rgba, ("bt709", "limited")))


# ---- 5. the command line ----

def test_cli_writes_one_y4m_file(tmp_path):
    def run(*args):
        p = subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout
    out = str(tmp_path / "out.y4m")
    run("-F", "3", "-s", "17x9", SWIRL, out)
    data = open(out, "rb").read()
    want = mm.Filter(SWIRL).invoke(17, 9).render_clip(num_frames=3)
    assert data.startswith(b"YUV4MPEG2 W17 H9 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
    fields, frames = X.parse_y4m(data)
    assert fields == {"W": "17", "H": "9", "F": "25:1", "I": "p", "A": "1:1", "C": "420jpeg", "XCOLORRANGE": "LIMITED"}
    assert np.array_equal(frames, X.frames(want, ("bt709", "limited")))
    assert data == X.y4m_file(frames, 17, 9)
    assert [p.name for p in tmp_path.iterdir()] == ["out.y4m"]
    # the same stream on standard output, in batches of two frames
    assert run("-F", "3", "--batch-frames=2", "-s", "17x9", SWIRL, "-") == data
    # the other mode, a frame rate, an anti-aliased clip
    out = str(tmp_path / "full.y4m")
    run("-F", "3", "-s", "64x8", "--aa=2", "--yuv-matrix=bt601", "--yuv-range=full", "--fps=30000:1001", SWIRL, out)
    data = open(out, "rb").read()
    want = mm.Filter(SWIRL).invoke(64, 8).render_clip(num_frames=3, aa=2)
    assert data.startswith(b"YUV4MPEG2 W64 H8 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n")
    fields, frames = X.parse_y4m(data)
    assert np.array_equal(frames, X.frames(want, ("bt601", "full")))
    assert data == X.y4m_file(frames, 64, 8, (30000, 1001), "full")
    # -F 1 (and no -F at all) gives a one-frame file
    for extra in (["-F", "1"], []):
        out = str(tmp_path / "one.y4m")
        run(*extra, "-s", "17x9", SWIRL, out)
        fields, frames = X.parse_y4m(open(out, "rb").read())
        assert frames.shape == (1, X.frame_bytes(17, 9))
        assert np.array_equal(frames, X.frames(mm.Filter(SWIRL).invoke(17, 9).render_clip(num_frames=1), ("bt709", "limited")))
