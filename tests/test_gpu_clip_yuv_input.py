"""Planar Y'CbCr 4:2:0 clip input on the GPU (mmhip_clip_from_yuv420: k_yuv420_to_rgba_clip on frames that stay in HBM,
mmhip_set_image_sequence_yuv420_host, read_y4m and the command line's .y4m inputs).

The yardstick is tests/yuv_input_reference.py.  Everything is compared byte for byte in whole sentinel-filled destination
buffers: in front of the first frame, between frames and behind the last frame nothing may change."""
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
from tests import yuv_input_reference as R
from tests import yuv_reference as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
SENTINEL = 0xA5
LEAD = 64                    # sentinel bytes in front of the first and behind the last frame (keeps the base 16-byte aligned)
PLAIN = "filter plain (image in) in(xy, frame) end"
BENT = "filter bent (image in) in(xy * 1.3 + xy:[0.11, -0.07], frame) end"
BLUR = "filter blur (image in)\n  b = gaussian_blur(in, 0.04, 0.06);\n  b(xy)\nend"
IDENTITY = "filter identity (image in) in(xy, frame) end"
CASES = [(mode, chroma) for mode in R.MODES for chroma in R.CHROMAS]


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
    array = np.ascontiguousarray(array, np.uint8)
    p = lib().mmhip_device_alloc(array.nbytes)
    assert p
    assert lib().mmhip_copy_to_device(C.c_void_p(p), array.ctypes.data_as(C.c_void_p), array.nbytes) == 0
    return p


def device_read(p, total):
    out = np.empty(total, np.uint8)
    assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), total) == 0
    return out


def convert(inv, yuv, w, h, mode, chroma, src_offset=0, src_gap=0, dst_gap=0, dst_offset=0):
    """Runs the converter over the payloads yuv [N, frame_bytes], which lie src_offset bytes into their buffer and src_gap
    bytes further apart than a frame (the padding holds 0x5A), and returns the whole destination buffer: LEAD + dst_offset
    sentinel bytes, the frames dst_gap bytes apart, LEAD more."""
    n, fb = yuv.shape
    assert fb == R.frame_bytes(w, h)
    buf = np.full(src_offset + n * (fb + src_gap) + 16, 0x5A, np.uint8)
    for i in range(n):
        at = src_offset + i * (fb + src_gap)
        buf[at:at + fb] = yuv[i]
    dstride = 4 * w * h + dst_gap
    total = LEAD + dst_offset + n * dstride + LEAD
    src, dst = upload(buf), device_filled(total)
    try:
        rc = lib().mmhip_clip_from_yuv420(inv._h, C.c_void_p(src + src_offset), fb + src_gap, w, h, n, R.MATRIX_IDS[mode[0]], R.RANGE_IDS[mode[1]],
                                          R.CHROMA_IDS[chroma], C.c_void_p(dst + LEAD + dst_offset), dstride, None)
        assert rc == 0, err()
        inv.sync()
        return device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


def expected(yuv, w, h, mode, chroma, dst_gap=0, dst_offset=0):
    """The destination buffer convert() must return: the restatement's words, the sentinel everywhere else."""
    n = len(yuv)
    frame = 4 * w * h
    want = np.full(LEAD + dst_offset + n * (frame + dst_gap) + LEAD, SENTINEL, np.uint8)
    word = R.words(R.rgba_frames(yuv, w, h, mode, chroma)).astype("<u4")
    for i in range(n):
        at = LEAD + dst_offset + i * (frame + dst_gap)
        want[at:at + frame] = word[i].reshape(-1).view(np.uint8)
    return want


def random_payloads(n, w, h, seed):
    """Every byte value in every plane: out-of-range samples and the clamps are exercised."""
    return np.random.default_rng(seed).integers(0, 256, (n, R.frame_bytes(w, h)), dtype=np.uint8)


def launches(inv):
    return inv.clip_from_yuv420_launches("aligned"), inv.clip_from_yuv420_launches("bytes")


# ---- 1. the converter alone ----

SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 5), (7, 3), (8, 2), (16, 2), (24, 4), (9, 2), (15, 6), (17, 9), (31, 33), (64, 8), (65, 7), (97, 61)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_converter_equals_the_restatement(inv, size):
    w, h = size
    for n in (1, 3):
        yuv = random_payloads(n, w, h, 100 * w + h + n)
        for mode, chroma in CASES:
            got = convert(inv, yuv, w, h, mode, chroma)
            assert np.array_equal(got, expected(yuv, w, h, mode, chroma)), (size, n, mode, chroma)


@pytest.mark.parametrize("size", [(64, 8), (24, 4)], ids=lambda s: "%dx%d" % s)
def test_both_paths_give_the_same_words(inv, size):
    """The path of wide accesses at aligned pointers and strides; the path of byte accesses with the source base 1 byte
    off, with the source frames 4 bytes further apart, and with the destination frames 4 bytes further apart or 4 off."""
    w, h = size
    yuv = random_payloads(3, w, h, 7)
    for mode, chroma in CASES:
        want = expected(yuv, w, h, mode, chroma)
        before = launches(inv)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma), want), (mode, chroma)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, src_offset=8, src_gap=8), want), (mode, chroma)
        assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, dst_gap=16, dst_offset=16), expected(yuv, w, h, mode, chroma, 16, 16)), (mode, chroma)
        aligned = launches(inv)
        assert aligned == (before[0] + 3, before[1])
        for case in (dict(src_offset=1), dict(src_offset=4), dict(src_gap=4), dict(src_gap=1)):
            assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, **case), want), (mode, chroma, case)
        for case in (dict(dst_gap=4), dict(dst_offset=4), dict(dst_offset=8)):
            assert np.array_equal(convert(inv, yuv, w, h, mode, chroma, **case), expected(yuv, w, h, mode, chroma, **case)), (mode, chroma, case)
        assert launches(inv) == (aligned[0], aligned[1] + 7)
    assert lib().mmhip_clip_from_yuv420_launches(inv._h, 2) == -1 and "path must be" in err()


def test_the_store_flavours_give_the_same_words():
    """MMHIP_YUV_IN_STORES is read per call: non-temporal stores on both paths, in a child process."""
    child = ("import sys, hashlib; sys.path.insert(0, %r)\n"
             "from tests import test_gpu_clip_yuv_input as T\n"
             "import mathmap_amd as mm\n"
             "inv = mm.Filter('filter f () rgba:[t, 0, 0, 1] end').invoke(8, 8)\n"
             "yuv = T.random_payloads(3, 64, 8, 7)\n"
             "for mode, chroma in T.CASES:\n"
             "    for case in ({}, dict(src_offset=1)):\n"
             "        got = T.convert(inv, yuv, 64, 8, mode, chroma, **case)\n"
             "        assert (got == T.expected(yuv, 64, 8, mode, chroma)).all(), (mode, chroma, case)\n"
             "print('launches', *T.launches(inv))\n") % ROOT
    env = dict(os.environ, MMHIP_YUV_IN_STORES="nt")
    r = subprocess.run([sys.executable, "-c", child], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "launches 8 8"


# ---- 2. every (Y, Cb, Cr) triple ----

@pytest.fixture(scope="module")
def every_triple():
    """4096 x 4096 in replicate mode: block b = 2048 (y >> 1) + (x >> 1) has Cb = (b >> 6) & 255 and Cr = b >> 14, its four
    pixels the lumas 4 (b & 63) + 2 (y & 1) + (x & 1): all 2^24 triples, once each."""
    b = np.arange(1 << 22, dtype=np.uint32).reshape(2048, 2048)
    cb, cr = ((b >> 6) & 255).astype(np.uint8), (b >> 14).astype(np.uint8)
    base = (4 * (b & 63)).astype(np.uint8)
    y = np.repeat(np.repeat(base, 2, axis=0), 2, axis=1)
    y[1::2] += 2
    y[:, 1::2] += 1
    triples = (y.astype(np.uint32) << 16 | np.repeat(np.repeat(cb, 2, 0), 2, 1).astype(np.uint32) << 8 | np.repeat(np.repeat(cr, 2, 0), 2, 1)).reshape(-1)
    seen = np.zeros(1 << 24, bool)
    seen[triples] = True
    assert seen.all()
    return y, cb, cr


@pytest.mark.parametrize("mode", R.MODES, ids="-".join)
def test_every_triple(inv, every_triple, mode):
    w = h = 4096
    y, cb, cr = every_triple
    payload = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    assert payload.size == R.frame_bytes(w, h)
    total = 4 * w * h + LEAD
    src, dst = upload(payload), device_filled(total)
    try:
        before = launches(inv)
        assert lib().mmhip_clip_from_yuv420(inv._h, C.c_void_p(src), payload.size, w, h, 1, R.MATRIX_IDS[mode[0]], R.RANGE_IDS[mode[1]],
                                            R.CHROMA_IDS["replicate"], C.c_void_p(dst), 4 * w * h, None) == 0, err()
        inv.sync()
        assert launches(inv) == (before[0] + 1, before[1])
        got = device_read(dst, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))
    assert (got[4 * w * h:] == SENTINEL).all()
    word = got[:4 * w * h].view("<u4").reshape(h, w)
    for r0 in range(0, h, 512):                         # (the restatement works in int64: a slice of rows at a time)
        u = np.repeat(np.repeat(cb[r0 // 2:(r0 + 512) // 2], 2, 0), 2, 1)
        v = np.repeat(np.repeat(cr[r0 // 2:(r0 + 512) // 2], 2, 0), 2, 1)
        r, g, b = R.matrix(y[r0:r0 + 512], u, v, mode)
        want = (r << 24 | g << 16 | b << 8 | 255).astype(np.uint32)
        assert np.array_equal(word[r0:r0 + 512], want), r0


# ---- 3. strides and refusals ----

@pytest.mark.parametrize("size", [(17, 9), (64, 8)], ids=lambda s: "%dx%d" % s)
def test_larger_frame_strides_leave_the_gaps_alone(inv, size):
    w, h = size
    yuv = random_payloads(3, w, h, 33)
    for src_gap, dst_gap in ((1, 4), (8, 16), (24, 1000), (1000, 0), (0, 48)):
        for mode, chroma in ((("bt601", "full"), "bilinear"), (("bt709", "limited"), "replicate")):
            got = convert(inv, yuv, w, h, mode, chroma, src_gap=src_gap, dst_gap=dst_gap)
            assert np.array_equal(got, expected(yuv, w, h, mode, chroma, dst_gap=dst_gap)), (src_gap, dst_gap, mode, chroma)


def test_the_call_refuses_by_name_and_writes_nothing(inv):
    w, h = 17, 9
    fb, frame = R.frame_bytes(w, h), 4 * w * h
    src, dst = upload(random_payloads(2, w, h, 5)), device_filled(2 * frame)
    try:
        def call(src=src, stride=fb, w=w, h=h, n=2, matrix=1, rng=0, chroma=0, dst=dst, dstride=frame):
            return lib().mmhip_clip_from_yuv420(inv._h, C.c_void_p(src), stride, w, h, n, matrix, rng, chroma, C.c_void_p(dst), dstride, None)
        for keywords, message in ((dict(w=0), "clip_from_yuv420: width and height must be at least 1, not 0 x 9"),
                                  (dict(h=0), "clip_from_yuv420: width and height must be at least 1, not 17 x 0"),
                                  (dict(n=0), "clip_from_yuv420: num_frames must be at least 1"),
                                  (dict(n=65536), "clip_from_yuv420: more than 65535 frames in one call (65536); convert the clip in groups"),
                                  (dict(matrix=2), "clip_from_yuv420: matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not 2"),
                                  (dict(rng=-1), "clip_from_yuv420: range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not -1"),
                                  (dict(chroma=2), "clip_from_yuv420: chroma must be MMHIP_YUV_CHROMA_BILINEAR or MMHIP_YUV_CHROMA_REPLICATE (0 or 1), not 2"),
                                  (dict(src=None), "clip_from_yuv420: src_yuv and dst_rgba32 must be device pointers"),
                                  (dict(dst=None), "clip_from_yuv420: src_yuv and dst_rgba32 must be device pointers"),
                                  (dict(stride=fb - 1), "clip_from_yuv420: src_frame_stride 242 is smaller than one frame (243 bytes)"),
                                  (dict(dstride=frame + 2), "clip_from_yuv420: dst_frame_stride 614 is not a multiple of 4"),
                                  (dict(dstride=frame - 4), "clip_from_yuv420: dst_frame_stride 608 is smaller than one frame (612 bytes)"),
                                  (dict(w=32768, h=32769, stride=1 << 40, dstride=1 << 40), "clip_from_yuv420: a destination frame of more than 4 GiB")):
            assert call(**keywords) == -1 and err() == message, keywords
        inv.sync()
        assert (device_read(dst, 2 * frame) == SENTINEL).all()
        assert call() == 0
    finally:
        inv.sync()
        lib().mmhip_device_free(C.c_void_p(src))
        lib().mmhip_device_free(C.c_void_p(dst))


# ---- 4. the host setter ----

SETTER_SIZES = [(17, 9, 5), (64, 8, 3)]


@pytest.mark.parametrize("source", [PLAIN, BENT], ids=["plain", "bent"])
@pytest.mark.parametrize("size", SETTER_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_a_yuv_bound_sequence_renders_what_the_rgba_bound_one_renders(size, source):
    w, h, n = size
    yuv = random_payloads(n, w, h, 50 + w)
    flt = mm.Filter(source)
    for mode, chroma in ((("bt709", "limited"), "bilinear"), (("bt601", "full"), "replicate")):
        rgba = R.rgba_frames(yuv, w, h, mode, chroma)
        inv = flt.invoke(w, h)
        if mode == ("bt709", "limited"):
            inv.set_image_yuv420("in", yuv, w, h)                        # the defaults
        else:
            inv.set_image_yuv420("in", yuv, w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        assert inv.clip_yuv_input_groups() == 1
        frames = [inv.render(t=0.1 * k, frame=k) for k in range(n + 1)]          # (frame n: the sequence has none, white)
        clip = inv.render_clip(num_frames=n)
        inv.set_image("in", rgba)
        for k in range(n + 1):
            assert np.array_equal(frames[k], inv.render(t=0.1 * k, frame=k)), (mode, chroma, k)
        assert np.array_equal(clip, inv.render_clip(num_frames=n)), (mode, chroma)
        if source == PLAIN:
            assert np.array_equal(clip, rgba) and (frames[n] == 255).all()
        # and back: a YUV upload replaces an RGBA one; one frame without the first axis is a single image
        inv.set_image_yuv420("in", yuv[1], w, h, yuv_matrix=mode[0], yuv_range=mode[1], chroma=chroma)
        single = inv.render(t=0.3, frame=0)
        inv.set_image("in", rgba[1])
        assert np.array_equal(single, inv.render(t=0.3, frame=0))


CHILD = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
import mathmap_amd as mm
from tests import test_gpu_clip_yuv_input as T
inv = mm.Filter(T.BENT).invoke(17, 9)
inv.enable_timing()
inv.set_image_yuv420("in", T.random_payloads(5, 17, 9, 67), 17, 9)
labels = [name for name, ms in inv.drain_native_kernel_ms()]
out = inv.render_clip(num_frames=5)
print(json.dumps({"groups": inv.clip_yuv_input_groups(), "labels": labels, "sha": hashlib.sha256(out.tobytes()).hexdigest()}))
"""


def test_groups_leave_the_words_alone():
    """MMHIP_CLIP_YUV_IN_BYTES holds two 17 x 9 payloads: 5 frames go up in 3 groups (the budget is read per call, in a child)."""
    env = dict(os.environ, MMHIP_CLIP_YUV_IN_BYTES=str(2 * R.frame_bytes(17, 9) + 100))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["groups"] == 3 and res["labels"].count("yuv420_to_rgba_clip") == 3
    yuv = random_payloads(5, 17, 9, 67)
    inv = mm.Filter(BENT).invoke(17, 9)
    inv.enable_timing()
    inv.set_image_yuv420("in", yuv, 17, 9)
    assert inv.clip_yuv_input_groups() == 1 and [name for name, ms in inv.drain_native_kernel_ms()].count("yuv420_to_rgba_clip") == 1
    single = inv.render_clip(num_frames=5)
    assert res["sha"] == hashlib.sha256(single.tobytes()).hexdigest()
    inv.set_image("in", R.rgba_frames(yuv, 17, 9, ("bt709", "limited"), "bilinear"))
    assert np.array_equal(single, inv.render_clip(num_frames=5))


def free_device_bytes():
    """hipMemGetInfo of the HIP runtime this process has loaded."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_rebinding_frees_the_earlier_upload():
    """512 x 512 x 32: a sequence of 32 MiB.  Twelve rebinds that kept theirs would hold 384 MiB."""
    w, h, n = 512, 512, 32
    yuv = random_payloads(n, w, h, 3)
    inv = mm.Filter(PLAIN).invoke(w, h)
    inv.set_image_yuv420("in", yuv, w, h)
    first = inv.render(frame=7)
    inv.sync()
    before = free_device_bytes()
    for k in range(12):
        inv.set_image_yuv420("in", yuv[::-1] if k % 2 == 0 else yuv, w, h)
    inv.sync()
    assert before - free_device_bytes() < 3 * (n * w * h * 4)
    assert np.array_equal(inv.render(frame=7), first)
    assert np.array_equal(first, R.rgba_frame(yuv[7], w, h, ("bt709", "limited"), "bilinear"))


def test_a_native_filter_reads_the_current_frame_of_a_yuv_bound_sequence():
    w, h, n = 64, 40, 3
    yuv = random_payloads(n, w, h, 91)
    flt = mm.Filter(BLUR)
    a, b = flt.invoke(w, h), flt.invoke(w, h)
    a.set_image_yuv420("in", yuv, w, h)
    b.set_image("in", R.rgba_frames(yuv, w, h, ("bt709", "limited"), "bilinear"))
    for v in (a, b):
        v.set_native_input_frame("current")
    for k in range(n):
        assert np.array_equal(a.render(t=0.2, frame=k), b.render(t=0.2, frame=k)), k
    assert np.array_equal(a.render_clip(num_frames=n), b.render_clip(num_frames=n))
    assert not np.array_equal(a.render(t=0.2, frame=0), a.render(t=0.2, frame=2))
    with pytest.raises(mm.MathMapError, match="frame 3 is outside"):
        a.render(frame=3)


# ---- 5. end to end ----

def block_clip(n, w, h, seed):
    """uint8 [n, h, w, 4]: 2 x 2 blocks of one random colour each, opaque."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, (n, h // 2, w // 2, 4), dtype=np.uint8)
    blocks[..., 3] = 255
    return np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2)


def test_out_through_a_file_and_in_again(tmp_path):
    """render_clip(yuv420p) -> write_y4m -> read_y4m -> set_image_yuv420 -> render_clip(yuv420p) through the identity
    filter at full range with replicate chroma, on 2 x 2-constant blocks: the planes come back within the round trip's
    bound of 1 (tests/test_clip_yuv_input_api.py states it)."""
    w, h, n = 64, 8, 3
    clip = block_clip(n, w, h, 8)
    inv = mm.Filter(IDENTITY).invoke(w, h)
    inv.set_image("in", clip)
    first = inv.render_clip(num_frames=n, pixel_format="yuv420p", yuv_range="full")
    assert np.array_equal(first, X.frames(clip, ("bt709", "full")))
    path = str(tmp_path / "clip.y4m")
    mm.api.write_y4m(path, first, w, h, fps=(24, 1), yuv_range="full")
    yuv, gw, gh, fps, yuv_range = mm.api.read_y4m(path)
    assert (gw, gh, fps, yuv_range) == (w, h, (24, 1), "full") and np.array_equal(yuv, first)
    inv.set_image_yuv420("in", yuv, gw, gh, yuv_range=yuv_range, chroma="replicate")
    back = inv.render_clip(num_frames=n)
    assert np.array_equal(back, R.rgba_frames(first, w, h, ("bt709", "full"), "replicate"))
    assert np.abs(back[..., :3].astype(int) - clip[..., :3].astype(int)).max() <= 1
    second = inv.render_clip(num_frames=n, pixel_format="yuv420p", yuv_range="full")
    diff = np.abs(second.astype(int) - first.astype(int))
    print("planes after the round trip: max %d" % diff.max())
    assert diff.max() <= 1


def test_cli_reads_a_y4m_file_and_a_pipe(tmp_path):
    w, h, n = 17, 9, 4
    yuv = random_payloads(n, w, h, 77)
    src = str(tmp_path / "in.y4m")
    mm.api.write_y4m(src, yuv, w, h, fps=(30000, 1001), yuv_range="full")

    def run(*args, stdin=None):
        p = subprocess.run([CLI] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout
    # size, frame count, frame rate and the input's range come from the stream; the output's range is its own option
    out = str(tmp_path / "out.y4m")
    run("-Din=" + src, PLAIN, out)
    rgba = R.rgba_frames(yuv, w, h, ("bt709", "full"), "bilinear")
    want = X.y4m_file(X.frames(rgba, ("bt709", "limited")), w, h, (30000, 1001), "limited")
    assert open(out, "rb").read() == want
    # the same through a pipe, in and out
    assert run("-Din=-", PLAIN, "-", stdin=open(src, "rb").read()) == want
    # the options of the input side; --input-frames caps the frames read, -F and --fps win over the stream's
    out = str(tmp_path / "other.y4m")
    run("-Din=" + src, "--input-frames=3", "--input-yuv-matrix=bt601", "--input-yuv-range=limited", "--input-chroma=replicate", "--yuv-range=full", PLAIN, out)
    rgba = R.rgba_frames(yuv[:3], w, h, ("bt601", "limited"), "replicate")
    assert open(out, "rb").read() == X.y4m_file(X.frames(rgba, ("bt709", "full")), w, h, (30000, 1001), "full")
    out = str(tmp_path / "two.y4m")
    run("-Din=" + src, "-F", "2", "--fps=25", "--input-chroma=replicate", PLAIN, out)
    rgba = R.rgba_frames(yuv[:2], w, h, ("bt709", "full"), "replicate")
    assert open(out, "rb").read() == X.y4m_file(X.frames(rgba, ("bt709", "limited")), w, h, (25, 1), "limited")
    # a header that does not state the range is limited
    bare = str(tmp_path / "bare.y4m")
    open(bare, "wb").write(b"YUV4MPEG2 W17 H9\n" + b"".join(b"FRAME Ip\n" + p.tobytes() for p in yuv[:2]))
    out = str(tmp_path / "bare_out.y4m")
    run("-Din=" + bare, PLAIN, out)
    rgba = R.rgba_frames(yuv[:2], w, h, ("bt709", "limited"), "bilinear")
    assert open(out, "rb").read() == X.y4m_file(X.frames(rgba, ("bt709", "limited")), w, h, (25, 1), "limited")
