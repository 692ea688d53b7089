"""10-bit planar Y'CbCr 4:2:0 clip input on the GPU (mmhip_clip_from_yuv420p10: k_yuv420p10_to_float_clip on frames that
stay in HBM, mmhip_set_image_sequence_yuv420p10_host, read_y4m and the command line's C420p10 inputs).

The yardstick is tests/yuv10_input_reference.py.  Everything is compared bit for bit (the floats as their 32-bit words) in
whole sentinel-filled destination buffers: in front of the first frame, between frames and behind the last frame nothing
may change."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from tests import yuv10_input_reference as R
from tests import yuv10_reference as X
from tests import yuv_input_reference as R8
from tests import yuv_reference as X8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
SENTINEL = 0xA5
LEAD = 64                    # sentinel bytes in front of the first and behind the last frame (keeps the base 16-byte aligned)
PLAIN = "filter plain (image in) in(xy, frame) end"
BENT = "filter bent (image in) in(xy * 1.3 + xy:[0.11, -0.07], frame) end"
BLUR = "filter blur (image in)\n  b = gaussian_blur(in, 0.04, 0.06);\n  b(xy)\nend"
CASES = [(mode, chroma) for mode in R.MODES for chroma in R.CHROMAS]
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (7, 3), (8, 2), (16, 2), (24, 4), (9, 2), (15, 6), (17, 9), (31, 33), (64, 8), (65, 7), (97, 61)]


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


def source_buffer(yuv, src_offset=0, src_gap=0):
    """The payloads yuv uint16 [N, samples] as bytes, src_offset bytes into the buffer and src_gap bytes further apart than
    a frame; the padding holds 0x5A."""
    n, samples = yuv.shape
    fb = 2 * samples
    buf = np.full(src_offset + n * (fb + src_gap) + 16, 0x5A, np.uint8)
    for i in range(n):
        at = src_offset + i * (fb + src_gap)
        buf[at:at + fb] = yuv[i].astype("<u2").view(np.uint8)
    return buf


def convert(inv, yuv, w, h, mode, chroma, src_offset=0, src_gap=0, dst_gap=0, dst_offset=0):
    """Runs the converter over the payloads and returns the whole destination buffer: LEAD + dst_offset sentinel bytes,
    the frames dst_gap bytes apart, LEAD more."""
    n, samples = yuv.shape
    assert samples == R.frame_samples(w, h)
    dstride = 16 * w * h + dst_gap
    total = LEAD + dst_offset + n * dstride + LEAD
    src, dst = upload(source_buffer(yuv, src_offset, src_gap)), device_filled(total)
    try:
        rc = lib().mmhip_clip_from_yuv420p10(inv._h, C.c_void_p(src + src_offset), 2 * samples + src_gap, w, h, n, R.MATRIX_IDS[mode[0]],
                                             R.RANGE_IDS[mode[1]], R.CHROMA_IDS[chroma], C.c_void_p(dst + LEAD + dst_offset), dstride, None)
        assert rc == 0, err()
        inv.sync()
        return device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


_FRAMES = {}


def reference(yuv, w, h, mode, chroma):
    """R.float_frames, computed once per input and shared."""
    key = (yuv.tobytes(), w, h, mode, chroma)
    if key not in _FRAMES:
        _FRAMES[key] = R.float_frames(yuv, w, h, mode, chroma)
        _FRAMES[key].setflags(write=False)
    return _FRAMES[key]


def expected(yuv, w, h, mode, chroma, dst_gap=0, dst_offset=0):
    """The destination buffer convert() must return: the restatement's floats, the sentinel everywhere else."""
    n = len(yuv)
    frame = 16 * w * h
    want = np.full(LEAD + dst_offset + n * (frame + dst_gap) + LEAD, SENTINEL, np.uint8)
    floats = reference(yuv, w, h, mode, chroma).astype("<f4")
    for i in range(n):
        at = LEAD + dst_offset + i * (frame + dst_gap)
        want[at:at + frame] = floats[i].reshape(-1).view(np.uint8)
    return want


def random_payloads(n, w, h, seed):
    """Every 16-bit value in every plane: what lies above 10 bits is read as 1023."""
    return np.random.default_rng(seed).integers(0, 65536, (n, R.frame_samples(w, h))).astype(np.uint16)


def legal_payloads(n, w, h, seed):
    return np.random.default_rng(seed).integers(0, 1024, (n, R.frame_samples(w, h))).astype(np.uint16)


def launches(inv):
    return inv.clip_from_yuv420p10_launches("aligned"), inv.clip_from_yuv420p10_launches("samples")


# ---- 1. the converter alone ----

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_converter_equals_the_restatement(inv, size):
    w, h = size
    before = launches(inv)
    for n in (1, 3):
        yuv = random_payloads(n, w, h, 100 * w + h + n)
        for mode, chroma in CASES:
            got = convert(inv, yuv, w, h, mode, chroma)
            assert np.array_equal(got, expected(yuv, w, h, mode, chroma)), (size, n, mode, chroma)
    # a width that is a multiple of 8 takes the aligned path (device allocations are aligned), every other the other one
    ran = 2 * len(CASES)
    assert launches(inv) == ((before[0] + ran, before[1]) if w % 8 == 0 else (before[0], before[1] + ran))


@pytest.mark.parametrize("size", [(64, 8), (24, 4)], ids=lambda s: "%dx%d" % s)
def test_both_paths_give_the_same_floats(inv, size):
    """The path of wide accesses at aligned pointers and strides, whatever the gaps between destination frames; the path
    of 2-byte loads with the source base 2 or 8 bytes off and with the source frames 2 or 8 bytes further apart."""
    w, h = size
    yuv = random_payloads(3, w, h, 7)
    for mode, chroma in CASES:
        want = expected(yuv, w, h, mode, chroma)
        before = launches(inv)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma), want), (mode, chroma)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, src_offset=16, src_gap=32), want), (mode, chroma)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, dst_gap=16, dst_offset=48), expected(yuv, w, h, mode, chroma, 16, 48)), (mode, chroma)
        aligned = launches(inv)
        assert aligned == (before[0] + 3, before[1])
        for case in (dict(src_offset=2), dict(src_offset=8), dict(src_gap=2), dict(src_gap=8), dict(src_offset=6, src_gap=10, dst_gap=32)):
            gaps = {k: v for k, v in case.items() if k.startswith("dst")}
            assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, **case), expected(yuv, w, h, mode, chroma, **gaps)), (mode, chroma, case)
        assert launches(inv) == (aligned[0], aligned[1] + 5)
    assert lib().mmhip_clip_from_yuv420p10_launches(inv._h, 2) == -1 and "path must be" in err()


@pytest.mark.parametrize("columns", ["2", "4", "8"])
@pytest.mark.parametrize("stores", ["cached", "nt"])
def test_the_switches_give_the_same_floats(inv, monkeypatch, columns, stores):
    """MMHIP_YUV10_IN_COLUMNS and MMHIP_YUV10_IN_STORES are read per call: every value of each, on both paths, at a width
    that is 8 times an odd number, at one with a single work-item per row pair, and over more than one workgroup."""
    monkeypatch.setenv("MMHIP_YUV10_IN_COLUMNS", columns)
    monkeypatch.setenv("MMHIP_YUV10_IN_STORES", stores)
    for w, h in ((24, 5), (8, 2), (128, 34)):
        yuv = random_payloads(2, w, h, 11)
        before = launches(inv)
        for mode, chroma in CASES:
            want = expected(yuv, w, h, mode, chroma)
            assert np.array_equal(convert(inv, yuv, w, h, mode, chroma), want), (w, h, mode, chroma)
            assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, src_offset=2), want), (w, h, mode, chroma)
        assert launches(inv) == (before[0] + len(CASES), before[1] + len(CASES))


# ---- 2. strides and refusals ----

@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_larger_frame_strides_leave_the_gaps_alone(inv, size):
    w, h = size
    yuv = random_payloads(3, w, h, 33)
    for src_gap, dst_gap in ((2, 16), (16, 32), (24, 1008), (1000, 0), (0, 48)):
        for mode, chroma in ((("bt601", "full"), "bilinear"), (("bt709", "limited"), "replicate")):
            got = convert(inv, yuv, w, h, mode, chroma, src_gap=src_gap, dst_gap=dst_gap)
            assert np.array_equal(got, expected(yuv, w, h, mode, chroma, dst_gap=dst_gap)), (src_gap, dst_gap, mode, chroma)


def test_the_call_refuses_by_name_and_writes_nothing(inv):
    w, h = 17, 9
    fb, frame = R.frame_bytes(w, h), 16 * w * h
    src, dst = upload(random_payloads(2, w, h, 5)), device_filled(2 * frame)
    try:
        def call(src=src, stride=fb, w=w, h=h, n=2, matrix=1, rng=0, chroma=0, dst=dst, dstride=frame):
            return lib().mmhip_clip_from_yuv420p10(inv._h, C.c_void_p(src), stride, w, h, n, matrix, rng, chroma, C.c_void_p(dst), dstride, None)
        assert fb == 486 and frame == 2448
        for keywords, message in ((dict(w=0), "width and height must be at least 1, not 0 x 9"),
                                  (dict(h=0), "width and height must be at least 1, not 17 x 0"),
                                  (dict(n=0), "num_frames must be at least 1"),
                                  (dict(n=65536), "more than 65535 frames in one call (65536); convert the clip in groups"),
                                  (dict(matrix=2), "matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not 2"),
                                  (dict(rng=-1), "range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not -1"),
                                  (dict(chroma=2), "chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not 2"),
                                  (dict(src=None), "src_yuv and dst_float4 must be device pointers"),
                                  (dict(dst=None), "src_yuv and dst_float4 must be device pointers"),
                                  (dict(src=src + 1), "src_yuv and src_frame_stride must be even (the samples are 16-bit)"),
                                  (dict(stride=fb + 1), "src_yuv and src_frame_stride must be even (the samples are 16-bit)"),
                                  (dict(stride=fb - 2), "src_frame_stride 484 is smaller than one frame (486 bytes)"),
                                  (dict(dst=dst + 8), "dst_float4 is not 16-byte aligned (float4 texels)"),
                                  (dict(dstride=frame + 8), "dst_frame_stride 2456 is not a multiple of 16"),
                                  (dict(dstride=frame - 16), "dst_frame_stride 2432 is smaller than one frame (2448 bytes)"),
                                  (dict(w=16384, h=16385, stride=1 << 40, dstride=1 << 40), "a destination frame of more than 4 GiB")):
            assert call(**keywords) == -1 and err() == "clip_from_yuv420p10: " + message, keywords
        inv.sync()
        assert (device_read(dst, 2 * frame) == SENTINEL).all()
        assert call() == 0
    finally:
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


# ---- 3. the host setter ----

def float_maps(inv, n):
    """render_clip(floatmap=True) of whole frames into device memory, read back: float32 [n, h, w, 4]."""
    w, h = inv.render_width, inv.render_height
    dev = lib().mmhip_device_alloc(n * w * h * 16)
    assert dev
    try:
        inv.render_clip(num_frames=n, floatmap=True, out_ptr=dev)
        inv.sync()
        out = np.empty((n, h, w, 4), np.float32)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes) == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    return out


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("source", [PLAIN, BENT], ids=["plain", "bent"])
@pytest.mark.parametrize("size", [(17, 9, 5), (64, 8, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_a_yuv_bound_sequence_renders_what_the_float_bound_one_renders(size, source):
    """End to end: set_image_yuv420p10 against set_image(the restatement's float32 frames), as float maps and as 10-bit
    planes."""
    w, h, n = size
    yuv = random_payloads(n, w, h, 50 + w)
    flt = mm.Filter(source, deep_inputs=True, intersample=source != PLAIN)      # (the plain one fetches the nearest texel: an identity)
    for mode, chroma in ((("bt709", "limited"), "bilinear"), (("bt601", "full"), "replicate")):
        frames = reference(yuv, w, h, mode, chroma)
        inv = flt.invoke(w, h)
        if mode == ("bt709", "limited"):
            inv.set_image_yuv420p10("in", yuv, w, h)                        # the defaults
        else:
            inv.set_image_yuv420p10("in", yuv, w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        assert inv.clip_yuv10_input_groups() == 1
        maps, planes, bytes8 = float_maps(inv, n), inv.render_clip(num_frames=n, pixel_format="yuv420p10"), inv.render_clip(num_frames=n)
        inv.set_image("in", np.array(frames))
        assert same(maps, float_maps(inv, n)), (mode, chroma)
        assert planes.dtype == np.uint16 and np.array_equal(planes, inv.render_clip(num_frames=n, pixel_format="yuv420p10")), (mode, chroma)
        assert np.array_equal(bytes8, inv.render_clip(num_frames=n))
        if source == PLAIN:
            assert same(maps, frames)                                       # nothing was clamped on the way in or out
        # and back: a YUV upload replaces a float one; one frame without the first axis is a single image
        inv.set_image_yuv420p10("in", yuv[1], w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        single = float_maps(inv, 1)
        inv.set_image("in", np.array(frames[1]))
        assert same(single, float_maps(inv, 1))


def test_groups_and_strided_payloads_leave_the_floats_alone(monkeypatch):
    """MMHIP_CLIP_YUV_IN_BYTES (read per call) holds two 17 x 9 payloads: 5 frames go up in 3 groups, one launch each;
    payloads 10 bytes further apart than a frame go up one by one."""
    w, h, n = 17, 9, 5
    yuv = random_payloads(n, w, h, 67)
    want = reference(yuv, w, h, ("bt601", "limited"), "bilinear")
    inv = mm.Filter(PLAIN, deep_inputs=True).invoke(w, h)
    inv.enable_timing()
    inv.set_image_yuv420p10("in", yuv, w, h, yuv_matrix="bt601")
    assert inv.clip_yuv10_input_groups() == 1 and [name for name, ms in inv.drain_native_kernel_ms()].count("yuv420p10_to_float_clip") == 1
    assert same(float_maps(inv, n), want)
    monkeypatch.setenv("MMHIP_CLIP_YUV_IN_BYTES", str(2 * R.frame_bytes(w, h) + 100))
    before = launches(inv)
    inv.set_image_yuv420p10("in", yuv[::-1], w, h, yuv_matrix="bt601")
    assert inv.clip_yuv10_input_groups() == 3 and [name for name, ms in inv.drain_native_kernel_ms()].count("yuv420p10_to_float_clip") == 3
    assert launches(inv) == (before[0], before[1] + 3)
    assert same(float_maps(inv, n), want[::-1])
    fb = R.frame_bytes(w, h)
    padded = np.full((n, fb // 2 + 5), 0xFFFF, np.uint16)
    padded[:, :fb // 2] = yuv
    index = inv._index("in")["index"]
    assert lib().mmhip_set_image_sequence_yuv420p10_host(inv._h, index, padded.ctypes.data_as(C.c_void_p), fb + 10, w, h, n, 0, 0, 0) == 0, err()
    assert inv.clip_yuv10_input_groups() == 3
    assert same(float_maps(inv, n), want)
    for stride, words in ((fb + 1, "frame_stride 487 is odd (the samples are 16-bit)"), (fb - 2, "frame_stride 484 is smaller than one frame (486 bytes)")):
        assert lib().mmhip_set_image_sequence_yuv420p10_host(inv._h, index, padded.ctypes.data_as(C.c_void_p), stride, w, h, n, 0, 0, 0) == -1
        assert err() == "set_image_sequence_yuv420p10_host: " + words
    assert lib().mmhip_set_image_sequence_yuv420p10_host(inv._h, index, padded.ctypes.data_as(C.c_void_p), fb + 10, w, h, n, 0, 0, 2) == -1
    assert err().startswith("clip_from_yuv420p10: chroma must be")
    assert same(float_maps(inv, n), want)                                   # what was bound stays bound


def test_a_filter_without_deep_inputs_is_refused_and_nothing_gets_bound():
    w, h = 17, 9
    yuv = legal_payloads(2, w, h, 4)
    inv = mm.Filter(PLAIN).invoke(w, h)
    unbound = inv.render()
    before = launches(inv)
    with pytest.raises(mm.MathMapError, match="set_image_sequence_yuv420p10_host: filter `plain' was not compiled with deep_inputs"):
        inv.set_image_yuv420p10("in", yuv, w, h)
    assert launches(inv) == before and np.array_equal(inv.render(), unbound)
    rgba = R8.rgba_frames(np.random.default_rng(1).integers(0, 256, (2, R8.frame_bytes(w, h)), dtype=np.uint8), w, h, ("bt709", "limited"), "bilinear")
    inv.set_image("in", rgba)
    bound = inv.render_clip(num_frames=2)
    with pytest.raises(mm.MathMapError, match="was not compiled with deep_inputs"):
        inv.set_image_yuv420p10("in", yuv, w, h)
    assert np.array_equal(inv.render_clip(num_frames=2), bound) and np.array_equal(bound, rgba)


def test_a_native_filter_refuses_the_image_by_name():
    w, h = 64, 40
    inv = mm.Filter(BLUR, deep_inputs=True).invoke(w, h)
    inv.set_image_yuv420p10("in", legal_payloads(1, w, h, 9), w, h)
    with pytest.raises(mm.MathMapError, match="gaussian_blur: float inputs are not supported by native filters"):
        inv.render()


# ---- 4. round trips ----

@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_grey_ramps_come_back_unchanged(mode):
    """Every legal luma code at chroma 512 in, the identity filter with the nearest fetch, the same matrix and range out:
    the Y plane is the one that went in and every chroma sample is 512."""
    lo, hi = (64, 940) if mode[1] == "limited" else (0, 1023)
    w, h = 64, 16
    codes = np.minimum(lo + np.arange(w * h), hi).astype(np.uint16)
    assert set(range(lo, hi + 1)) <= set(codes.tolist())
    yuv = np.concatenate([codes, np.full(2 * (w // 2) * (h // 2), 512, np.uint16)])[None]
    inv = mm.Filter(PLAIN, intersample=False, deep_inputs=True).invoke(w, h)
    for chroma in R.CHROMAS:
        inv.set_image_yuv420p10("in", yuv, w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        back = inv.render_clip(num_frames=1, pixel_format="yuv420p10", yuv_matrix=mode[0], yuv_range=mode[1])
        y, cb, cr = mm.api.yuv420_planes(back, w, h)
        assert np.array_equal(y.reshape(-1), codes), (mode, chroma)
        assert (cb == 512).all() and (cr == 512).all(), (mode, chroma)


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_a_coloured_frame_of_blocks_is_the_two_restatements_chained(mode):
    w, h, n = 64, 8, 2
    blocks = np.random.default_rng(8).random((n, h // 2, w // 2, 4), dtype=np.float32)
    first = X.frames(np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2), mode)
    inv = mm.Filter(PLAIN, intersample=False, deep_inputs=True).invoke(w, h)
    inv.set_image_yuv420p10("in", first, w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma="replicate")
    second = inv.render_clip(num_frames=n, pixel_format="yuv420p10", yuv_matrix=mode[0], yuv_range=mode[1])
    assert np.array_equal(second, X.frames(reference(first, w, h, mode, "replicate"), mode))
    moved = np.abs(second.astype(int) - first.astype(int)).max()
    print("planes after out -> in -> out: max %d" % moved)


# ---- 5. the command line ----

def test_cli_reads_a_10_bit_y4m_file_and_a_pipe(tmp_path):
    w, h, n = 17, 9, 4
    yuv = random_payloads(n, w, h, 77)
    src = str(tmp_path / "in.y4m")
    mm.api.write_y4m(src, yuv, w, h, fps=(30000, 1001), yuv_range="full")

    def run(*args, stdin=None, ok=True):
        p = subprocess.run([CLI] + list(args), input=stdin, stdin=None if stdin is not None else subprocess.DEVNULL, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout if ok else p.stderr.decode()

    def python_path(source, frames, mode, chroma, out_mode, **options):
        inv = mm.Filter(source, deep_inputs=True, **options).invoke(w, h)
        inv.set_image_yuv420p10("in", frames, w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        return inv.render_clip(num_frames=len(frames), pixel_format="yuv420p10", yuv_matrix=out_mode[0], yuv_range=out_mode[1])
    # size, frame count, frame rate and the input's range come from the stream; the output's range is its own option
    out = str(tmp_path / "out.y4m")
    run("-Din=" + src, "--pixel-format=yuv420p10", PLAIN, out)
    planes = python_path(PLAIN, yuv, ("bt709", "full"), "bilinear", ("bt709", "limited"), intersample=False)
    want = X.y4m_file(planes, w, h, (30000, 1001), "limited")
    assert open(out, "rb").read() == want
    assert np.array_equal(planes, X.frames(reference(yuv, w, h, ("bt709", "full"), "bilinear"), ("bt709", "limited")))
    # the same through a pipe, in and out
    assert run("-Din=-", "--pixel-format=yuv420p10", PLAIN, "-", stdin=open(src, "rb").read()) == want
    # the options of the input side; --input-frames caps the frames read; -i is the bilinear fetch
    out = str(tmp_path / "other.y4m")
    run("-i", "-Din=" + src, "--input-frames=3", "--input-yuv-matrix=bt601", "--input-yuv-range=limited", "--input-chroma=replicate", "--yuv-range=full",
        "--pixel-format=yuv420p10", BENT, out)
    planes = python_path(BENT, yuv[:3], ("bt601", "limited"), "replicate", ("bt709", "full"), intersample=True)
    assert open(out, "rb").read() == X.y4m_file(planes, w, h, (30000, 1001), "full")
    # a 10-bit input and an 8-bit output
    out = str(tmp_path / "eight.y4m")
    run("-Din=" + src, PLAIN, out)
    inv = mm.Filter(PLAIN, intersample=False, deep_inputs=True).invoke(w, h)
    inv.set_image_yuv420p10("in", yuv, w, h, yuv_range="full")
    assert open(out, "rb").read() == X8.y4m_file(inv.render_clip(num_frames=n, pixel_format="yuv420p"), w, h, (30000, 1001), "limited")
    # a native filter that reads the image fails with the runtime's message
    assert "gaussian_blur: float inputs are not supported by native filters" in run("-Din=" + src, BLUR, str(tmp_path / "blur.y4m"), ok=False)
    # an 8-bit input gives the bytes it gave before
    yuv8 = np.random.default_rng(78).integers(0, 256, (n, R8.frame_bytes(w, h)), dtype=np.uint8)
    src8 = str(tmp_path / "in8.y4m")
    mm.api.write_y4m(src8, yuv8, w, h, fps=(24, 1), yuv_range="full")
    out = str(tmp_path / "out8.y4m")
    run("-Din=" + src8, PLAIN, out)
    rgba = R8.rgba_frames(yuv8, w, h, ("bt709", "full"), "bilinear")
    want8 = X8.y4m_file(X8.frames(rgba, ("bt709", "limited")), w, h, (24, 1), "limited")
    assert open(out, "rb").read() == want8
    assert run("-Din=-", PLAIN, "-", stdin=open(src8, "rb").read()) == want8
