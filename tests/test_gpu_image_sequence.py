"""Multi-frame input drawables on the GPU: in(xy, n) reads frame (int)n of a sequence.

The oracle binds one frame per image and only range-checks the frame number, so every expected frame is composed from
oracle renders: for a frame number inside the sequence, the same filter with the literal 0 in its place and that frame
bound as its single image; for one outside, the filter with that number and any image -- the oracle's own range check
then gives the white frame with the edge colours on top.  A pixel-dependent number picks, pixel by pixel, among those
renders by an index map the oracle renders too.  The probes' arithmetic is affine (tests/sequence_probes.py): every
comparison is byte for byte."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import sequence_probes as P
from tests.gpu_util import render_device

pytestmark = pytest.mark.gpu
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
K = 5
IW, IH = 83, 61             # the frames of the sequence
W, H = 160, 121             # the rendered frame: another size, and odd, so that y = 0 on its centre row
INT_MIN = -(1 << 31)
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mathmap_amd", "mathmap_hip_cli")


def noise(k=K, w=IW, h=IH, seed=7, channels=4):
    return np.random.default_rng(seed).integers(0, 256, (k, h, w, channels), dtype=np.uint8)


_ORACLES = {}


def oracle(src):
    if src not in _ORACLES:
        _ORACLES[src] = CpuFilter(mm.Filter(src).ir_json_raw)
    return _ORACLES[src]


def expected_frame(template, n, seq, w=W, h=H, **kw):
    """What the fetches of `template` at frame number n (an int) of `seq` give: see the module's text."""
    if 0 <= n < len(seq):
        return oracle(P.text(template, "0")).render(w, h, images={"in": seq[n]}, **kw)
    return oracle(P.text(template, str(n))).render(w, h, images={"in": seq[0]}, **kw)


def first_difference(got, want):
    bad = np.argwhere(np.any(got != want, axis=-1))
    return None if not len(bad) else (tuple(int(v) for v in bad[0]), len(bad))


def assert_same(got, want, what):
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), (what, first_difference(got, want))


def bound(src, seq, w=W, h=H, uservals=None, **opts):
    flt = mm.Filter(src, **opts)
    inv = flt.invoke(w, h)
    inv.set_image("in", seq)
    for k, v in (uservals or {}).items():
        inv.set(k, v)
    return flt, inv


FRAME_NUMBERS = (-1, 0, 2, K - 1, K)


# ---- 1. frame-constant selection ----

@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("kind", ["frame", "userval"])
def test_frame_constant_selection(kind, intersample):
    seq = noise()
    src = P.text(P.SELECT, P.FRAME_OF_ANIMATION if kind == "frame" else P.FRAME_OF_USERVAL)
    flt, inv = bound(src, seq, intersample=intersample)
    for n in FRAME_NUMBERS:
        if kind == "userval":
            inv.set("n", n + 8)
        frame = n if kind == "frame" else 0
        got = render_device(inv, W, H, t=0.3, frame=frame)
        want = expected_frame(P.SELECT, n, seq, t=0.3, frame=frame, intersample=intersample)
        assert_same(got, want, (kind, intersample, n))
    # the frames differ from each other and from the white frame: the comparison above told them apart
    a, b, white = (expected_frame(P.SELECT, n, seq, intersample=intersample) for n in (0, 2, K))
    assert not np.array_equal(a, b) and not np.array_equal(a, white)
    assert (white == 255).all(axis=-1).any() and not (white == 255).all()      # white inside, edge colour (0) outside


@pytest.mark.parametrize("edge", [(1, 2), (2, 3), (3, 1), (0, 0)], ids=["wrap-reflect", "reflect-rotate", "rotate-wrap", "color-color"])
@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
def test_edge_behaviours_and_colours_come_before_the_frame_test(edge, intersample):
    seq = noise(seed=11)
    colors = (0x11223344, 0xa0b0c0d0)
    src = P.text(P.SELECT, P.FRAME_OF_ANIMATION)
    flt, inv = bound(src, seq, intersample=intersample, edge_x=edge[0], edge_y=edge[1])
    inv.set_edge_colors(*colors)
    for n in (-1, 2, K):
        got = render_device(inv, W, H, frame=n)
        want = expected_frame(P.SELECT, n, seq, frame=n, intersample=intersample, edge=edge, edge_colors=colors)
        assert_same(got, want, (edge, intersample, n))
    if edge == (0, 0):      # an edge colour wins over a frame that does not exist
        out = expected_frame(P.SELECT, K, seq, frame=K, intersample=False, edge=edge, edge_colors=colors)
        assert (out[0, 0] == (0x11, 0x22, 0x33, 0x44)).all() and (out[0, W // 2] == (0xa0, 0xb0, 0xc0, 0xd0)).all()
        assert (out[H // 2, W // 2] == 255).all()


def test_strided_source():
    seq = noise(seed=13)
    flt, inv = bound(P.text(P.SELECT, P.FRAME_OF_ANIMATION), seq, intersample=True, pixel_inc=3)
    for n in (2, K):
        assert_same(render_device(inv, W, H, frame=n), expected_frame(P.SELECT, n, seq, frame=n, pixel_inc=3), n)
    flt, inv = bound(P.text(P.SLIT, P.SLIT_FRAME), seq, intersample=True, pixel_inc=3)
    assert_same(render_device(inv, W, H), expected_slit(seq, {}, W, H, intersample=True, pixel_inc=3), "slit")


def test_bands_regions_and_float_maps():
    seq = noise(seed=17)
    flt, inv = bound(P.text(P.SELECT, P.FRAME_OF_ANIMATION), seq)
    for n in (3, K):
        want = expected_frame(P.SELECT, n, seq, frame=n)
        assert_same(render_device(inv, W, H, frame=n, rows=[(0, 17), (17, 60), (60, H)]), want, ("bands", n))
        rx, ry, rw, rh = 21, 9, 100, 77
        dev = lib().mmhip_device_alloc(rw * rh * 4)
        assert dev
        try:
            inv.render_rows(dev, ry, ry + rh, frame=n, region=(rx, ry, rw, rh))
            inv.sync()
            got = np.empty((rh, rw, 4), np.uint8)
            assert lib().mmhip_copy_to_host(got.ctypes.data_as(C.c_void_p), C.c_void_p(dev), got.nbytes) == 0
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
        assert_same(got, want[ry:ry + rh, rx:rx + rw], ("region", n))
        assert_same(render_device(inv, W, H, frame=n, floatmap=True), expected_frame(P.SELECT, n, seq, frame=n, floatmap=True),
                    ("float map", n))


# ---- 2. in(xy) reads frame (int)t ----

def test_plain_fetch_reads_frame_int_t():
    seq = noise(seed=19)
    flt, inv = bound(P.PLAIN, seq)
    assert_same(render_device(inv, W, H, t=0.25), expected_frame(P.SELECT, 0, seq, t=0.25), "t = 0.25")
    assert_same(render_device(inv, W, H, t=1.0), expected_frame(P.SELECT, 1, seq, t=1.0), "t = 1.0")
    # a single image at t = 1.0 has no frame 1: white, as the oracle has it
    flt, inv = bound(P.PLAIN, seq[0])
    want = oracle(P.PLAIN).render(W, H, images={"in": seq[0]}, t=1.0)
    assert_same(render_device(inv, W, H, t=1.0), want, "single image, t = 1.0")
    assert_same(want, expected_frame(P.SELECT, K, seq), "white frame")


# ---- 3. pixel-dependent frame numbers ----

def c_int_cast(f):
    """(int)f of a float32 array as x86-64 converts it: toward zero; NaN and out of range give INT_MIN."""
    out = np.full(f.shape, INT_MIN, np.int64)
    ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    out[ok] = np.trunc(f[ok]).astype(np.int64)
    return out


def slit_index(seq, uservals, w, h, index_src=P.SLIT_INDEX):
    fmap = oracle(index_src).render(w, h, uservals=uservals, images={"in": seq[0]}, floatmap=True, threads=THREADS)
    return c_int_cast(fmap[..., 0])


def expected_slit(seq, uservals, w, h, index=None, template=P.SLIT, **kw):
    index = slit_index(seq, uservals, w, h) if index is None else index
    want = oracle(P.text(template, "99")).render(w, h, uservals=uservals, images={"in": seq[0]}, threads=THREADS, **kw)
    for k in range(len(seq)):
        if (index == k).any():
            s = oracle(P.text(template, "0")).render(w, h, uservals=uservals, images={"in": seq[k]}, threads=THREADS, **kw)
            want[index == k] = s[index == k]
            del s
    return want


# off - 8 + k * (x + 1) (+ big * x * 1e14) + (NaN where y = 0), x in [-1, 1]
SLIT_CASES = {
    "spread": {"off": 8.0, "k": 1.75},             # 0 .. 3.5, NaN on the centre row
    "fractional": {"off": 7.5, "k": 0.375},        # -0.5 .. 0.25: all frame 0
    "beyond": {"off": 6.0, "k": 4.0},              # -2 .. 6: negative, and K and above
    "huge": {"off": 8.0, "k": 1.75, "big": 1.0},   # +-1e14 away from the centre column
}


def check_index_map(case, index):
    if case == "spread":
        assert (index[H // 2] == INT_MIN).all() and set(np.unique(np.delete(index, H // 2, 0))) == {0, 1, 2, 3}
    if case == "fractional":
        assert set(np.unique(np.delete(index, H // 2, 0))) == {0}
    if case == "beyond":
        assert index.min() == INT_MIN and (index == -1).any() and (index == K).any() and (index == K - 1).any()
    if case == "huge":
        assert (np.delete(index, H // 2, 0)[:, 1] == INT_MIN).all() and (np.delete(index, H // 2, 0)[:, -1] == INT_MIN).all()


def test_fractional_frame_number_reads_frame_zero():
    # -0.5 truncates toward zero: the oracle's own index map says so before anything is rendered
    seq = noise(seed=23)
    fmap = oracle(P.SLIT_INDEX).render(W, H, uservals=SLIT_CASES["fractional"], images={"in": seq[0]}, floatmap=True)
    assert fmap[0, 0, 0] == np.float32(-0.5)
    assert slit_index(seq, SLIT_CASES["fractional"], W, H)[0, 0] == 0


@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("path", ["hot", "frame_hot_off", "single_pixel"])
def test_pixel_dependent_frame_numbers(path, intersample, monkeypatch):
    """hot: the branch-free per-pixel fetch (mm_orig_val_hotf); frame_hot_off: the same kernel shape with the site on
    the early-exit fetch; single_pixel: the kernel shape of large bodies (one pixel per work-item, early-exit fetch)."""
    if path == "frame_hot_off":
        monkeypatch.setenv("MMHIP_FRAME_HOT", "0")
    if path == "single_pixel":
        monkeypatch.setenv("MMHIP_SINGLE_PIXEL", "1")
    seq = noise(seed=29)
    src = P.text(P.SLIT, P.SLIT_FRAME)
    flt, inv = bound(src, seq, intersample=intersample)
    geo = flt.launch_geometry(W, H)
    assert geo["single_pixel"] == (path == "single_pixel") and ("hotf(" in flt.kernel_source.split(" mm_pixels(mm_args A")[1]) == (path == "hot")
    assert path == "single_pixel" or geo["unroll"] == 4
    for case, uv in SLIT_CASES.items():
        index = slit_index(seq, uv, W, H)
        check_index_map(case, index)
        for k, v in {"off": 8.0, "k": 1.75, "big": 0.0, **uv}.items():
            inv.set(k, v)
        got = render_device(inv, W, H)
        assert_same(got, expected_slit(seq, uv, W, H, index=index, intersample=intersample), (path, intersample, case))


@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
def test_pixel_dependent_frame_number_in_a_large_body(intersample):
    """A filter the generator itself gives the large-body kernel (no hook): its fetch is the early-exit one."""
    seq = noise(seed=73)
    flt, inv = bound(P.text(P.LARGE, P.LARGE_FRAME), seq, intersample=intersample)
    assert flt.launch_geometry(W, H)["single_pixel"] and "mm_hot" not in flt.kernel_source.split(" mm_pixels(mm_args A")[1]
    for case in ("spread", "beyond"):
        uv = SLIT_CASES[case]
        for k, v in uv.items():
            inv.set(k, v)
        index = slit_index(seq, uv, W, H, index_src=P.LARGE_INDEX)
        assert (index[H // 2] == INT_MIN).all() and len(set(np.unique(index)) & set(range(K))) >= 4
        want = expected_slit(seq, uv, W, H, index=index, template=P.LARGE, intersample=intersample)
        assert_same(render_device(inv, W, H), want, (case, intersample))


def test_pixel_dependent_frame_numbers_at_more_rows_per_work_item(monkeypatch):
    """ppt > MM_UNROLL: the unrolled loop goes round more than once per work-item (the 8192^2 frame below gets there by
    its size; here MMHIP_PPT forces it on a small frame)."""
    monkeypatch.setenv("MMHIP_PPT", "12")
    seq = noise(seed=31)
    w, h = 333, 251
    flt, inv = bound(P.text(P.SLIT, P.SLIT_FRAME), seq, w=w, h=h, uservals=SLIT_CASES["beyond"])
    geo = flt.launch_geometry(w, h)
    assert geo["unroll"] == 4 and geo["ppt"] == 12 and not geo["single_pixel"], geo
    assert_same(render_device(inv, w, h), expected_slit(seq, SLIT_CASES["beyond"], w, h), geo)


# ---- 4. temporal blend ----

@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
def test_temporal_blend(intersample):
    seq = noise(seed=37)
    flt, inv = bound(P.BLEND, seq, intersample=intersample)
    for frame in (0, 2, K - 1, K + 3):
        taps = {"a": frame - 1, "b": frame, "c": frame + 1}
        src = P.BLEND_ORACLE
        for name, n in taps.items():
            src = src.replace("{%s}" % name.upper(), "0" if 0 <= n < K else "7")
        images = {name: seq[n if 0 <= n < K else 0] for name, n in taps.items()}
        want = oracle(src).render(W, H, images=images, frame=frame, intersample=intersample)
        assert_same(render_device(inv, W, H, frame=frame), want, (intersample, frame))


# ---- 5. other consumers ----

@pytest.mark.parametrize("template", [P.RECURSIVE, P.CLOSURE], ids=["recursive", "closure"])
def test_frame_argument_in_filter_functions_and_closures(template):
    seq = noise(seed=41, w=W, h=H)
    flt, inv = bound(P.text(template, "n - 8"), seq)
    for n in (-1, 0, 3, K):
        inv.set("n", n + 8)
        got = render_device(inv, W, H, t=0.4, frame=2)
        assert_same(got, expected_frame(template, n, seq, t=0.4, frame=2), n)


@pytest.mark.parametrize("src", [P.BLUR, P.RENDER, F.GAUSS_DIRECT], ids=["gaussian_blur", "render", "direct_blur"])
def test_native_filters_read_frame_zero(src):
    seq = noise(seed=43, w=W, h=H)
    uv = {"hdev": 0.03, "vdev": 0.02} if src is F.GAUSS_DIRECT else {}
    flt, inv = bound(src, seq, uservals=uv)
    before = inv.direct_native_launches()
    got = render_device(inv, W, H, t=0.7, frame=3)
    if src is F.GAUSS_DIRECT:
        assert inv.direct_native_launches() == before + 1
    want = oracle(src).render(W, H, uservals=uv, images={"in": seq[0]}, t=0.7, frame=3)
    assert_same(got, want, "frame 0")
    assert not np.array_equal(want, oracle(src).render(W, H, uservals=uv, images={"in": seq[3]}, t=0.7, frame=3))
    assert_same(render_device(inv, W, H, t=0.7, frame=3, floatmap=True),
                oracle(src).render(W, H, uservals=uv, images={"in": seq[0]}, t=0.7, frame=3, floatmap=True), "float map")


def test_tolerance_blur_reads_frame_zero():
    seq = noise(seed=47, w=256, h=256)
    uv = {"hdev": 0.03, "vdev": 0.02}
    flt, inv = bound(F.GAUSS_DIRECT, seq, w=256, h=256, uservals=uv, gauss_mode="tolerance")
    got = render_device(inv, 256, 256, frame=2)
    assert inv.tolerance_blur_launches() == 1
    want = oracle(F.GAUSS_DIRECT).render(256, 256, uservals=uv, images={"in": seq[0]}, frame=2)
    assert np.abs(got.astype(np.int16) - want.astype(np.int16)).max() <= 1      # the mode's own contract (mmhip.h)


# ---- 6. device binding ----

DEVICE_TENSOR_CHILD = """
import sys
import numpy as np
import torch                      # before the engine: one process, one HIP runtime, torch's first
import mathmap_amd as mm
from tests import sequence_probes as P
from tests.gpu_util import render_device
packed, out, w, h = np.load(sys.argv[1]), sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
tensor = torch.from_numpy(packed.view(np.int32)).cuda()
k, ih, iw = tensor.shape
inv = mm.Filter(P.text(P.SELECT, P.FRAME_OF_ANIMATION)).invoke(w, h)
inv.set_image_device("in", tensor.data_ptr(), iw, ih, keepalive=tensor, num_frames=k)
frames = [render_device(inv, w, h, frame=n) for n in (-1, 0, 2, k - 1, k)]
try:
    inv.set_image_device("in", tensor.data_ptr(), iw, ih, num_frames=0)
    raise SystemExit("num_frames = 0 was accepted")
except mm.MathMapError as e:
    assert "num_frames" in str(e), e
inv.set_image_device("in", tensor.data_ptr(), iw, ih, keepalive=tensor)      # without num_frames: one image, as before
frames.append(render_device(inv, w, h, frame=1))
np.save(out, np.stack(frames))
"""


def test_sequence_from_a_device_tensor(tmp_path):
    """(In a process of its own: torch has to initialise the GPU before the engine does.)"""
    seq = noise(seed=53)
    p = seq.astype(np.uint32)
    packed = (p[..., 0] << 24) | (p[..., 1] << 16) | (p[..., 2] << 8) | p[..., 3]
    assert packed.shape == (K, IH, IW)
    np.save(str(tmp_path / "packed.npy"), packed)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_TENSOR_CHILD, str(tmp_path / "packed.npy"), str(tmp_path / "frames.npy"), str(W), str(H)],
                       cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = np.load(str(tmp_path / "frames.npy"))
    for got, n in zip(frames, FRAME_NUMBERS):
        assert_same(got, expected_frame(P.SELECT, n, seq, frame=n), n)
    assert_same(frames[-1], expected_frame(P.SELECT, K, seq, frame=1), "one frame bound")


# ---- 7. rebinding ----

def test_rebinding_a_sequence_invalidates_a_memoised_blur():
    a, b = noise(seed=59, w=W, h=H), noise(k=3, seed=61, w=W, h=H)
    flt, inv = bound(P.BLUR, a)
    cf = oracle(P.BLUR)
    want_a, want_b = cf.render(W, H, images={"in": a[0]}), cf.render(W, H, images={"in": b[0]})
    assert not np.array_equal(want_a, want_b)
    assert_same(render_device(inv, W, H), want_a, "first")
    assert_same(render_device(inv, W, H), want_a, "memoised")
    inv.set_image("in", b)
    assert_same(render_device(inv, W, H), want_b, "rebound")
    # and the frame count is the new one: frame 3 of the first sequence is gone
    flt, inv = bound(P.text(P.SELECT, P.FRAME_OF_ANIMATION), a)
    assert_same(render_device(inv, W, H, frame=3), expected_frame(P.SELECT, 3, a, frame=3), "K = 5")
    inv.set_image("in", b)
    assert_same(render_device(inv, W, H, frame=3), expected_frame(P.SELECT, 3, b, frame=3), "K = 3")
    assert_same(render_device(inv, W, H, frame=2), expected_frame(P.SELECT, 2, b, frame=2), "K = 3")


# ---- 8. command line ----

def write_png(path, rgb):
    h, w, _ = rgb.shape

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))
    raw = b"".join(b"\0" + rgb[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def read_png(path):
    """The command line's own output: 8-bit RGB, every row's filter type 0."""
    data = open(path, "rb").read()
    at, idat, w, h = 8, b"", 0, 0
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (8, 2)
        if kind == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3).copy()


def test_cli_processes_a_clip_frame_by_frame(tmp_path):
    seq = noise(k=3, seed=67, channels=3)
    for k in range(3):
        write_png(str(tmp_path / ("in%02d.png" % k)), seq[k])
    src = P.text(P.SELECT, P.FRAME_OF_ANIMATION)
    p = subprocess.run([CLI, "--input-frames=3", "-F", "3", "-Din=%s" % (tmp_path / "in%02d.png"), src, str(tmp_path / "out%d.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    flt, inv = bound(src, seq, w=IW, h=IH, intersample=False)
    for k in range(3):
        t = float(np.float32(k) / np.float32(3))
        want = render_device(inv, IW, IH, t=t, frame=k)
        assert_same(read_png(str(tmp_path / ("out%d.png" % k))), want[..., :3], k)
        assert_same(want, expected_frame(P.SELECT, k, seq, w=IW, h=IH, t=t, frame=k, intersample=False), k)
    # a define without a conversion stays a single image: frames 1 and 2 of the output are white where the image is
    p = subprocess.run([CLI, "--input-frames=3", "-F", "3", "-Din=%s" % (tmp_path / "in01.png"), src, str(tmp_path / "one%d.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert_same(read_png(str(tmp_path / "one0.png")), expected_frame(P.SELECT, 0, seq[1:2], w=IW, h=IH, intersample=False)[..., :3], "one0")
    assert_same(read_png(str(tmp_path / "one2.png")), expected_frame(P.SELECT, 2, seq[1:2], w=IW, h=IH, frame=2, intersample=False)[..., :3], "one2")
    # a missing frame, and frames of another size
    p = subprocess.run([CLI, "--input-frames=4", "-Din=%s" % (tmp_path / "in%02d.png"), src, str(tmp_path / "bad.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 1 and "in03.png" in p.stderr, p.stderr
    write_png(str(tmp_path / "in02.png"), noise(k=1, w=IW + 1, seed=1, channels=3)[0])
    p = subprocess.run([CLI, "--input-frames=3", "-Din=%s" % (tmp_path / "in%02d.png"), src, str(tmp_path / "bad.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 1 and "one size" in p.stderr and "in02.png" in p.stderr, p.stderr

# ---- 9. one whole frame at the benchmark's size ----

def test_slit_scan_8192():
    size, k = 8192, 4
    seq = noise(k=k, w=size, h=size, seed=71)
    uv = {"off": 7.0, "k": 3.0}                   # -1 .. 5 over the frame: every frame, and none on both sides
    flt, inv = bound(P.text(P.SLIT, P.SLIT_FRAME), seq, w=size, h=size, uservals=uv, intersample=True)
    assert "hotf(" in flt.kernel_source.split(" mm_pixels(mm_args A")[1]
    geo = flt.launch_geometry(size, size)
    assert geo["unroll"] == 4 and geo["ppt"] > geo["unroll"], geo
    got = render_device(inv, size, size)
    del inv
    index = slit_index(seq, uv, size, size)
    assert set(np.unique(index)) == {-1, 0, 1, 2, 3, 4, 5}      # (even height: no row has y = 0)
    assert_same(got, expected_slit(seq, uv, size, size, index=index, intersample=True), "8192^2")
