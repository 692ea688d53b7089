"""Clip rendering on the GPU: one batched launch renders the frames mmhip_render gives one at a time.

The yardstick is the single-frame path of the same build: the clip kernels' bodies are the single-frame kernels' text under
the same compile options, so every comparison is byte for byte (float maps bit for bit), over the *whole* output buffer --
both sides start from the same sentinel bytes, so a byte written outside a band shows as well.  A subset is held against
the oracle too, which pins the yardstick itself."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from mathmap_amd.striping import animation_frame_t
from oracle.ccgen import CpuFilter
from tests import filters as F
from tests import sequence_probes as P
from tests.clip_probes import MEDIUM, WAVE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
W, H = 333, 207              # odd: partial tiles on both edges for every tile shape
SENTINEL = 0xA5
LEAD = 192                   # sentinel bytes in front of the first and behind the last frame
# neither consecutive nor monotone, with repeats and negative numbers
FRAMES = [5, -2, 0, 119, 3, 3, 60]
TS = [0.9, 0.1, 0.5, 0.0, 0.33, 0.34, 1.0]
RAND = "filter rnd (image in) in(xy) * 0.5 + grayColor(rand(0, 0.5)) end"


def make(src, w=W, h=H, uservals=None, image=None, **opts):
    flt = F.load(src, **opts) if src in F.NAMES else mm.Filter(src, **opts)
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        inv.set_image("in", F.synthetic_image(w, h, seed=5) if image is None else image)
    for k, v in (uservals or {}).items():
        inv.set(k, v)
    return flt, inv


class Buffers:
    """Two device buffers of `total` sentinel bytes: one for the clip, one for the loop of single renders."""

    def __init__(self, total):
        self.total = total
        fill = np.full(total, SENTINEL, np.uint8)
        self.ptrs = []
        for _ in range(2):
            p = lib().mmhip_device_alloc(total)
            assert p
            self.ptrs.append(p)
            assert lib().mmhip_copy_to_device(C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), total) == 0

    def read(self, k):
        out = np.empty(self.total, np.uint8)
        assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptrs[k]), self.total) == 0
        return out

    def free(self):
        for p in self.ptrs:
            lib().mmhip_device_free(C.c_void_p(p))


def clip_and_loop(inv, frames, ts, region=None, rows=None, bpp=4, floatmap=False, row_stride=None, frame_stride=None, what=""):
    """Renders the clip and, frame by frame, the same bands at the same places of a second buffer; asserts that the two
    buffers are equal, that nothing outside the bands was written and that the bands were.  Returns the clip's bands as
    [N, rows, region_w, channels]."""
    rw_full, rh_full = inv.render_width, inv.render_height
    rx, ry, rw, rh = region if region is not None else (0, 0, rw_full, rh_full)
    first, last = rows if rows is not None else (ry, ry + rh)
    n_rows = min(last, ry + rh) - max(first, 0)
    px = 16 if floatmap else bpp
    stride = 16 * rw_full if floatmap else (row_stride if row_stride is not None else rw * bpp)
    band = n_rows * stride if floatmap else (n_rows - 1) * stride + rw * bpp
    fstride = frame_stride if frame_stride is not None else n_rows * stride
    assert fstride >= band
    n = len(frames)
    bufs = Buffers(2 * LEAD + n * fstride)
    try:
        inv.render_clip(frames=frames, ts=ts, out_ptr=bufs.ptrs[0] + LEAD, rows=(first, last), region=(rx, ry, rw, rh), bpp=bpp,
                        floatmap=floatmap, row_stride=stride, frame_stride=fstride)
        inv.sync()
        for i in range(n):
            inv.render_rows(bufs.ptrs[1] + LEAD + i * fstride, first, last, t=float(ts[i]), frame=int(frames[i]), row_stride=stride,
                            bpp=bpp, floatmap=floatmap, region=(rx, ry, rw, rh))
        inv.sync()
        clip, loop = bufs.read(0), bufs.read(1)
    finally:
        bufs.free()
    inside = np.zeros(clip.size, bool)
    for i in range(n):
        for r in range(n_rows):
            at = LEAD + i * fstride + r * stride
            inside[at:at + rw * px] = True
    bad = np.flatnonzero(clip != loop)
    assert bad.size == 0, (what, "clip != loop of single renders", int(bad[0]), int(bad.size), "frame %d" % ((int(bad[0]) - LEAD) // fstride))
    assert (clip[~inside] == SENTINEL).all(), (what, "bytes outside the bands were written")
    assert (clip[inside] != SENTINEL).any(), (what, "nothing was written")
    bands = np.empty((n, n_rows, rw * px), np.uint8)
    for i in range(n):
        for r in range(n_rows):
            at = LEAD + i * fstride + r * stride
            bands[i, r] = clip[at:at + rw * px]
    return bands.view(np.float32).reshape(n, n_rows, rw, 4) if floatmap else bands.reshape(n, n_rows, rw, bpp)


def expected_launches(flt, region_w, num_rows, n):
    plan = flt.clip_batch_plan(region_w, num_rows, n)
    return plan["batches"], (1 if plan["shared_slot"] else n)


# ---- 1. one filter per kernel class, N = 1, 2, 7 ----

CLASS_CASES = [
    ("mandelbrot", "mandelbrot", {}),                                   # a loop, no fetch
    ("mandelbrot-specialised", "mandelbrot", {"specialize": True}),     # pair mode
    ("pond", "pond", {}),                                               # the prologue reads t
    ("droste", "droste", {}),                                           # the large-body kernel: one pixel per work-item
    ("ident", "ident", {}),
    ("medium", MEDIUM, {}),                                             # two pixels per step
    ("wave", WAVE, {}),                                                 # a per-row slice that reads t
    ("recursive_data", "recursive_data", {}),                           # filter functions
    ("recursive_mutual", "recursive_mutual", {}),                       # ... with rand() inside, which hashes the frame
    ("rand", RAND, {}),
]


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("case", CLASS_CASES, ids=[c[0] for c in CLASS_CASES])
def test_clip_equals_single_frames(case, n):
    name, src, opts = case
    flt, inv = make(src, **opts)
    got = clip_and_loop(inv, FRAMES[:n], TS[:n], what=(name, n))
    # the specialised variant is what rendered, if the filter specialises: its plan counts
    active = flt.specialized() if opts.get("specialize") else flt
    batches, pro = expected_launches(active, W, H, n)
    assert batches == 1
    assert inv.clip_batched_launches() == batches, name
    assert inv.clip_prologue_frames() == pro, name
    if n > 1 and name in ("pond", "wave", "rand", "recursive_mutual", "medium"):
        assert not np.array_equal(got[0], got[1]), name      # these read t or frame: the comparison told frames apart


def test_pair_mode_is_what_the_specialised_mandelbrot_runs():
    assert F.load("mandelbrot").specialized().clip_launch_geometry(W, H, 7)["pair_mode"] == 1


@pytest.mark.parametrize("name", ["ident", "pond", "mandelbrot"])
def test_120_frames_by_the_command_lines_convention(name):
    """num_frames=N alone: frame = i, t = (float)i / (float)N, as -F N renders."""
    w, h = 96, 64
    flt, inv = make(name, w, h)
    got = inv.render_clip(num_frames=120)
    assert got.shape == (120, h, w, 4) and got.dtype == np.uint8
    assert inv.clip_batched_launches() == 1
    assert inv.clip_prologue_frames() == (1 if flt.clip_batch_plan(w, h, 120)["shared_slot"] else 120)
    for i in range(120):
        want = inv.render(t=animation_frame_t(i, 120), frame=i)
        assert np.array_equal(got[i], want), (name, i)
    if name == "pond":
        assert not np.array_equal(got[0], got[60])


def test_shared_slot_filters_evaluate_their_constants_once():
    """Frame constants that read neither t nor frame: one slot, one prologue row for the whole call."""
    seq = np.random.default_rng(3).integers(0, 256, (1, 61, 83, 4), dtype=np.uint8)
    for name, src in (("mandelbrot", "mandelbrot"), ("select-0", P.text(P.SELECT, "0"))):
        flt, inv = make(src, image=seq)
        assert flt.clip_batch_plan(W, H, 7)["shared_slot"] == 1, name
        clip_and_loop(inv, FRAMES, TS, what=name)
        assert inv.clip_prologue_frames() == 1 and inv.clip_batched_launches() == 1, name
        clip_and_loop(inv, FRAMES[:3], TS[:3], what=name)
        assert inv.clip_prologue_frames() == 2 and inv.clip_batched_launches() == 2, name


# ---- 2. the yardstick itself, against the oracle ----

def test_clip_against_the_oracle():
    flt, inv = make("mandelbrot", 96, 64)
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    cf = CpuFilter(flt.ir_json_raw)
    for i in range(3):
        assert np.array_equal(got[i], cf.render(96, 64, t=TS[i], frame=FRAMES[i])), i
    img = F.synthetic_image(96, 64, seed=5)
    flt, inv = make("droste", 96, 64, image=img)
    got = inv.render_clip(frames=FRAMES[:2], ts=TS[:2])
    cf = CpuFilter(flt.ir_json_raw)
    for i in range(2):
        assert np.array_equal(got[i], cf.render(96, 64, images={"in": img}, t=TS[i], frame=FRAMES[i])), i
    flt, inv = make(WAVE, 96, 64, image=img)
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    cf = CpuFilter(flt.ir_json_raw)
    for i in range(3):
        assert np.array_equal(got[i], cf.render(96, 64, images={"in": img}, t=TS[i], frame=FRAMES[i])), i


# ---- 3. a clip in, a clip out: frame numbers that run out of the input's range inside the clip ----

K = 5
SEQ_FRAMES = [-1, 0, 2, K - 1, K, 7, 1]
SEQ_CASES = [
    ("select", P.text(P.SELECT, P.FRAME_OF_ANIMATION), {}),
    ("slit", P.text(P.SLIT, P.SLIT_FRAME + " + frame"), {"off": 6.0, "k": 2.0}),
    ("blend", P.BLEND, {}),
    ("large", P.text(P.LARGE, P.LARGE_FRAME + " + frame"), {}),
]


@pytest.mark.parametrize("intersample", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("case", SEQ_CASES, ids=[c[0] for c in SEQ_CASES])
def test_sequence_probes(case, intersample):
    name, src, uservals = case
    seq = np.random.default_rng(7).integers(0, 256, (K, 61, 83, 4), dtype=np.uint8)
    flt, inv = make(src, 160, 121, uservals=uservals, image=seq, intersample=intersample)
    ts = [0.0, 0.2, 3.5, 0.7, 1.0, 0.1, 0.6]
    got = clip_and_loop(inv, SEQ_FRAMES, ts, what=(name, intersample))
    assert inv.clip_batched_launches() == 1
    assert not np.array_equal(got[1], got[2]), name


def test_select_against_the_oracle():
    """in(xy, frame) of a 5-frame input: inside the sequence the oracle's render of that frame, outside the white frame."""
    seq = np.random.default_rng(7).integers(0, 256, (K, 61, 83, 4), dtype=np.uint8)
    flt, inv = make(P.text(P.SELECT, P.FRAME_OF_ANIMATION), 160, 121, image=seq)
    got = inv.render_clip(frames=SEQ_FRAMES, ts=[0.0] * len(SEQ_FRAMES))
    for i, n in enumerate(SEQ_FRAMES):
        if 0 <= n < K:
            want = CpuFilter(mm.Filter(P.text(P.SELECT, "0")).ir_json_raw).render(160, 121, images={"in": seq[n]}, frame=n)
        else:
            want = CpuFilter(mm.Filter(P.text(P.SELECT, str(n))).ir_json_raw).render(160, 121, images={"in": seq[0]}, frame=n)
        assert np.array_equal(got[i], want), n


# ---- 4. output shapes ----

@pytest.mark.parametrize("bpp", [1, 2, 3])
@pytest.mark.parametrize("name", ["pond", "mandelbrot"])
def test_bytes_per_pixel(name, bpp):
    flt, inv = make(name)
    clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=bpp, what=(name, bpp))
    # rows and frames apart by strides that are no multiple of the pixel size
    clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=bpp, row_stride=W * bpp + 5, frame_stride=H * (W * bpp + 5) + 77, what=(name, bpp, "padded"))


@pytest.mark.parametrize("name", ["pond", "mandelbrot", "droste", "wave"])
def test_float_maps(name):
    flt, inv = make(WAVE if name == "wave" else name)
    got = clip_and_loop(inv, FRAMES[:3], TS[:3], floatmap=True, what=name)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    # a band of a region: the rows stay the frame's render width apart
    clip_and_loop(inv, FRAMES[:3], TS[:3], floatmap=True, region=(21, 9, 100, 77), rows=(20, 60), frame_stride=40 * 16 * W + 4096, what=(name, "region"))


@pytest.mark.parametrize("name", ["pond", "ident", "mandelbrot-specialised", "droste", "wave"])
def test_band_of_an_offset_region_between_sentinels(name):
    src, opts = (("mandelbrot", {"specialize": True}) if name == "mandelbrot-specialised" else (WAVE if name == "wave" else name, {}))
    flt, inv = make(src, **opts)
    region = (21, 9, 235, 150)
    for rows in ((9, 159), (40, 41), (33, 120), (-5, 500)):      # (the last is clipped to rows 0 .. 159, like mmhip_render's)
        clip_and_loop(inv, FRAMES[:4], TS[:4], region=region, rows=rows, row_stride=235 * 4 + 52, frame_stride=160 * (235 * 4 + 52) + 1000,
                      what=(name, rows))


def test_small_and_thin_frames():
    for w, h in ((1, 1), (17, 5), (640, 3), (3, 300)):
        flt, inv = make("pond", w, h)
        clip_and_loop(inv, FRAMES, TS, what=("pond", w, h))
        flt, inv = make("mandelbrot", w, h, specialize=True)
        clip_and_loop(inv, FRAMES, TS, what=("mandelbrot", w, h))


# ---- 5. batches and forced geometry ----

CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_render_clip import make, clip_and_loop, FRAMES, TS, WAVE
out = {}
for name in ("pond", "mandelbrot", WAVE):
    flt, inv = make(name)
    clip_and_loop(inv, FRAMES, TS, what=name)
    out[name[:12]] = [flt.clip_batch_plan(333, 207, 7), inv.clip_batched_launches(), inv.clip_prologue_frames()]
    inv.enable_timing(True)
    inv.render_clip(frames=FRAMES, ts=TS)
    out[name[:12]].append(len(inv.drain_kernel_ms()))
print(json.dumps(out))
"""


def test_clip_max_frames_splits_a_clip_into_batches():
    """MMHIP_CLIP_MAX_FRAMES=3 (read once: a child process) on 7 frames: three batches, the same bytes."""
    env = dict(os.environ, MMHIP_CLIP_MAX_FRAMES="3")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(out) == 3
    for name, (plan, launches, prologue_frames, timed) in out.items():
        assert plan["frames_per_batch"] == 3 and plan["batches"] == 3, name
        assert launches == 3, name
        assert prologue_frames == (1 if plan["shared_slot"] else 7), name
        assert timed == 3, name      # one timed entry per batch


@pytest.mark.parametrize("ppt", ["1", "3", "8", "64"])
def test_forced_rows_per_item(ppt, monkeypatch):
    monkeypatch.setenv("MMHIP_PPT", ppt)
    for name in ("pond", "ident", "mandelbrot"):
        flt, inv = make(name, specialize=(name == "mandelbrot"))
        g = flt.clip_launch_geometry(W, H, 7)
        assert g["ppt"] == -(-int(ppt) // g["unroll"]) * g["unroll"]
        clip_and_loop(inv, FRAMES, TS, what=(name, ppt))
        clip_and_loop(inv, FRAMES[:2], TS[:2], region=(3, 2, 300, 200), rows=(7, 190), what=(name, ppt, "band"))


def test_timing_reports_one_entry_per_batch():
    flt, inv = make("pond")
    inv.enable_timing(True)
    inv.render_clip(frames=FRAMES, ts=TS)
    inv.render_clip(frames=FRAMES[:2], ts=TS[:2])
    ms = inv.drain_kernel_ms()
    assert len(ms) == 2 and all(m > 0 for m in ms)


# ---- 6. state: clip, single frame, clip on one invocation ----

@pytest.mark.parametrize("specialize", [False, True], ids=["generic", "specialised"])
def test_clip_single_clip_with_a_user_value_changed(specialize):
    """The single-frame path caches its prologue on the buffers the clip rewrites, and a changed user value means new
    tables (and, specialised, another kernel variant)."""
    img = F.synthetic_image(W, H, seed=5)
    flt, inv = make("pond", specialize=specialize)
    fresh = lambda **uv: make("pond", uservals=uv)[1]
    uv = [u for u in flt.uservals if u["kind"] == mm.api.UV_FLOAT][0]
    other = (uv["float_min"] + uv["float_default"]) / 2 if uv["float_default"] != uv["float_min"] else (uv["float_min"] + uv["float_max"]) / 2
    single = inv.render(t=0.5, frame=0)
    a = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    assert np.array_equal(inv.render(t=0.5, frame=0), single)                 # same arguments as before the clip: no stale prologue
    assert np.array_equal(a[2], single)                                       # FRAMES[2], TS[2] = 0, 0.5
    inv.set(uv["name"], other)
    changed = inv.render(t=0.5, frame=0)
    assert not np.array_equal(changed, single)
    b = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    assert np.array_equal(b[2], changed)
    ref = fresh(**{uv["name"]: other})
    for i in range(3):
        assert np.array_equal(b[i], ref.render(t=TS[i], frame=FRAMES[i])), i
    inv.set(uv["name"], uv["float_default"])
    c = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    assert np.array_equal(c, a)
    assert np.array_equal(inv.render(t=0.5, frame=0), single)
    assert inv.clip_batched_launches() == 3


def test_two_clips_in_flight_on_one_stream():
    """Asynchronous calls back to back: each keeps its own {t, frame} table until its kernels have read it."""
    flt, inv = make("pond")
    n = 3
    size = n * W * H * 4
    ptrs = [lib().mmhip_device_alloc(size) for _ in range(4)]
    assert all(ptrs)
    try:
        for k, p in enumerate(ptrs):
            inv.render_clip(frames=[f + k for f in FRAMES[:n]], ts=[t * 0.5 + 0.1 * k for t in TS[:n]], out_ptr=p)
        inv.sync()
        for k, p in enumerate(ptrs):
            got = np.empty((n, H, W, 4), np.uint8)
            assert lib().mmhip_copy_to_host(got.ctypes.data_as(C.c_void_p), C.c_void_p(p), size) == 0
            for i in range(n):
                assert np.array_equal(got[i], inv.render(t=TS[i] * 0.5 + 0.1 * k, frame=FRAMES[i] + k)), (k, i)
    finally:
        for p in ptrs:
            lib().mmhip_device_free(C.c_void_p(p))


# ---- 7. filters that need the host between prologue and pixels ----

@pytest.mark.parametrize("name", ["gauss_direct", "closure_timed_arg"])
def test_native_filters_fall_back_to_single_renders(name):
    flt, inv = make(name, 160, 121)
    assert flt.clip_batch_plan(160, 121, 3)["frames_per_batch"] == 0
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3])
    assert inv.clip_batched_launches() == 0 and inv.clip_prologue_frames() == 0
    flt2, ref = make(name, 160, 121)
    for i in range(3):
        assert np.array_equal(got[i], ref.render(t=TS[i], frame=FRAMES[i])), (name, i)
    if name == "closure_timed_arg":
        assert not np.array_equal(got[0], got[1])
    clip_and_loop(inv, FRAMES[:3], TS[:3], region=(5, 3, 120, 100), rows=(10, 90), what=name)


def test_render_clip_refuses_a_short_frame_stride_and_missing_arrays():
    flt, inv = make("mandelbrot", 64, 32)
    dev = lib().mmhip_device_alloc(64 * 32 * 16 * 2)
    try:
        with pytest.raises(mm.MathMapError, match="frame_stride"):
            inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], out_ptr=dev, frame_stride=64 * 32 * 4 - 1)
        with pytest.raises(mm.MathMapError, match="frame_stride"):
            inv.render_clip(frames=[0, 1], ts=[0.0, 0.5], out_ptr=dev, floatmap=True, frame_stride=64 * 32 * 16 - 1)
        with pytest.raises(mm.MathMapError, match="num_frames"):
            inv.render_clip(frames=[], ts=[], out_ptr=dev)
        with pytest.raises(mm.MathMapError):
            inv.render_clip(frames=[0, 1], ts=[0.0])
        assert inv.clip_batched_launches() == 0
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))


# ---- 8. the command line ----

def test_cli_batch_frames_writes_the_same_files(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a + t * 3), frame / 6, 1] end"
    runs = {"loop": [], "clip": ["--batch-frames=4"], "whole": ["--batch-frames=100"]}
    for tag, extra in runs.items():
        p = subprocess.run([CLI, "-F", "6", "-s", "97x61"] + extra + [src, str(tmp_path / (tag + "%d.png"))],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    files = [open(str(tmp_path / ("loop%d.png" % i)), "rb").read() for i in range(6)]
    assert len(set(files)) == 6      # the frames differ
    for tag in ("clip", "whole"):
        for i in range(6):
            assert open(str(tmp_path / ("%s%d.png" % (tag, i))), "rb").read() == files[i], (tag, i)
    p = subprocess.run([CLI, "-F", "6", "-s", "97x61", "--batch-frames=0", src, str(tmp_path / "bad%d.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 1 and "--batch-frames" in p.stderr
