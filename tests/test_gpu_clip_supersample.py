"""Supersampled clips on the GPU: mmhip_render_clip_supersampled writes the bytes the loop of mmhip_render_supersampled writes.

The yardstick is that loop, on the same build and the same invocation: two batched slice renders and one launch of the
clip combine kernel against two single renders and the single-frame combine per frame.  Both sides write into buffers
pre-filled with the same sentinel bytes and the *whole* buffers are compared, so a byte written between rows, between
frames or outside the region shows as well.  Two filters are held against the oracle too, which pins the yardstick."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib
from oracle.ccgen import CpuFilter, render_supersampled
from tests import filters as F
from tests import sequence_probes as P
from tests.clip_probes import MEDIUM, WAVE
from tests.expectations import Expectations

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
W, H = 333, 207              # W % 4 = 1: the last column group of a row holds one pixel
SENTINEL = 0xA5
LEAD = 192                   # sentinel bytes in front of the first and behind the last frame (a multiple of 16)
# neither consecutive nor monotone, with repeats and negative numbers
FRAMES = [5, -2, 0, 119, 3, 3, 60]
TS = [0.9, 0.1, 0.5, 0.0, 0.33, 0.34, 1.0]
EXPECT = Expectations("clip_supersample")


def make(src, w=W, h=H, uservals=None, image=None, supersampling=True, **opts):
    flt = F.load(src, supersampling=supersampling, **opts) if src in F.NAMES else mm.Filter(src, supersampling=supersampling, **opts)
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        inv.set_image("in", F.synthetic_image(w, h, seed=5) if image is None else image)
    for k, v in (uservals or {}).items():
        inv.set(k, v)
    return flt, inv


def int_array(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def float_array(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def clip_ss(inv, frames, ts, region, out_ptr, row_stride, frame_stride, bpp):
    rx, ry, rw, rh = region
    return lib().mmhip_render_clip_supersampled(inv._h, len(frames), int_array(frames), float_array(ts), rx, ry, rw, rh,
                                                C.c_void_p(out_ptr), row_stride, frame_stride, bpp, None)


def loop_ss(inv, frames, ts, region, out_ptr, row_stride, frame_stride, bpp):
    rx, ry, rw, rh = region
    for i in range(len(frames)):
        assert lib().mmhip_render_supersampled(inv._h, int(frames[i]), float(ts[i]), rx, ry, rw, rh,
                                               C.c_void_p(out_ptr + i * frame_stride), row_stride, bpp, None) == 0, mm.api._err()


def device_filled(total):
    p = lib().mmhip_device_alloc(total)
    assert p
    fill = np.full(total, SENTINEL, np.uint8)
    assert lib().mmhip_copy_to_device(C.c_void_p(p), fill.ctypes.data_as(C.c_void_p), total) == 0
    return p


def device_read(p, total):
    out = np.empty(total, np.uint8)
    assert lib().mmhip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), total) == 0
    return out


def clip_and_loop(inv, frames, ts, region=None, bpp=4, row_stride=None, frame_stride=None, offset=0, what=""):
    """Renders the supersampled clip and, frame by frame, the same frames at the same places of a second buffer; asserts
    that the two buffers are equal, that nothing outside the frames' rows was written and that the rows were.  `offset`
    shifts the first frame behind the (16-byte aligned) start of the buffers.  Returns the clip's frames as [N, h, w, bpp]."""
    rx, ry, rw, rh = region = region if region is not None else (0, 0, inv.render_width, inv.render_height)
    stride = row_stride if row_stride is not None else rw * bpp
    fstride = frame_stride if frame_stride is not None else rh * stride
    assert fstride >= (rh - 1) * stride + rw * bpp
    n = len(frames)
    total = 2 * LEAD + offset + n * fstride
    a, b = device_filled(total), device_filled(total)
    try:
        assert clip_ss(inv, frames, ts, region, a + LEAD + offset, stride, fstride, bpp) == 0, (what, mm.api._err())
        inv.sync()
        loop_ss(inv, frames, ts, region, b + LEAD + offset, stride, fstride, bpp)
        inv.sync()
        clip, loop = device_read(a, total), device_read(b, total)
    finally:
        lib().mmhip_device_free(C.c_void_p(a))
        lib().mmhip_device_free(C.c_void_p(b))
    inside = np.zeros(total, bool)
    out = np.empty((n, rh, rw * bpp), np.uint8)
    for i in range(n):
        for r in range(rh):
            at = LEAD + offset + i * fstride + r * stride
            inside[at:at + rw * bpp] = True
            out[i, r] = clip[at:at + rw * bpp]
    bad = np.flatnonzero(clip != loop)
    assert bad.size == 0, (what, "clip != loop of single supersampled renders", int(bad[0]), int(bad.size),
                           "frame %d" % ((int(bad[0]) - LEAD - offset) // fstride))
    assert (clip[~inside] == SENTINEL).all(), (what, "bytes outside the frames' rows were written")
    assert (clip[inside] != SENTINEL).any(), (what, "nothing was written")
    return out.reshape(n, rh, rw, bpp)


def aligned_layout(w, h, bpp=4):
    """Row and frame strides that are multiples of 16: with a 16-byte aligned buffer, the combine's 16-byte stores."""
    stride = (w * bpp + 15) // 16 * 16 + 16
    return dict(row_stride=stride, frame_stride=h * stride + 32)


# ---- 1. one filter per kernel class, N = 1, 2, 7 ----

SEQ = np.random.default_rng(7).integers(0, 256, (5, 61, 83, 4), dtype=np.uint8)
CLASS_CASES = [
    ("ident", "ident", {}, None),
    ("pond", "pond", {}, None),                                             # the prologue reads t
    ("mandelbrot-specialised", "mandelbrot", {"specialize": True}, None),   # pair mode
    ("droste", "droste", {}, None),                                         # the large-body kernel
    ("wave", WAVE, {}, None),                                               # a per-row slice that reads t: two row tables
    ("medium", MEDIUM, {}, None),                                           # two pixels per step
    ("select-frame", P.text(P.SELECT, P.FRAME_OF_ANIMATION), {}, SEQ),      # in(xy, frame) of a 5-frame input
]


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("case", CLASS_CASES, ids=[c[0] for c in CLASS_CASES])
def test_clip_equals_the_loop_of_supersampled_renders(case, n):
    name, src, opts, image = case
    flt, inv = make(src, image=image, **opts)
    got = clip_and_loop(inv, FRAMES[:n], TS[:n], what=(name, n))                          # rows of 1332 bytes: dword stores
    clip_and_loop(inv, FRAMES[:n], TS[:n], what=(name, n, "aligned"), **aligned_layout(W, H))   # 16-byte stores
    active = flt.specialized() if opts.get("specialize") else flt
    plan = active.clip_supersample_plan(W, H, n)
    assert plan["batched"] == 1 and plan["batches"] == 1 and plan["frames_per_batch"] == n
    assert inv.clip_supersampled_batches() == 2, name
    assert inv.clip_batched_launches() == 4, name                                          # two slices per batch
    if n > 1 and name in ("pond", "wave", "medium"):
        assert not np.array_equal(got[0], got[1]), name      # these read t or frame: the comparison told frames apart
    if n == 7 and name == "select-frame":
        assert not np.array_equal(got[2], got[4]), name      # frames 0 and 3 of the input (5 and -2 are both outside it)


def test_pair_mode_is_what_the_specialised_mandelbrot_runs():
    assert F.load("mandelbrot", supersampling=True).specialized().clip_launch_geometry(W + 1, H, 7)["pair_mode"] == 1


# ---- 2. the smallest shapes where the combine can go wrong ----

def shape_cases():
    plan = F.load("pond", supersampling=True).clip_supersample_plan(37, 37, 3)
    r, k = plan["rows_per_item"], plan["pixels_per_item"]
    sizes = [(1, 1), (2, 3), (3, 1), (4, 2), (5, 7), (64, 1), (67, 33)]
    sizes += [(37, h) for h in (r - 1, r, r + 1, 2 * r + 1)]                 # around one strip of rows, and a third strip of one row
    sizes += [(w, r + 2) for w in (k - 1, k, k + 1)]                          # around one column group
    sizes += [(w, r + 2) for w in (64 * k - 1, 64 * k, 64 * k + 1)]           # around one wave of column groups
    return sizes


@pytest.fixture(scope="module")
def pond_filter():
    return F.load("pond", supersampling=True)


@pytest.mark.parametrize("size", shape_cases(), ids=lambda s: "%dx%d" % s)
def test_small_shapes(pond_filter, size):
    w, h = size
    inv = pond_filter.invoke(w, h)
    inv.set_image("in", F.synthetic_image(w, h, seed=5))
    clip_and_loop(inv, FRAMES[:3], TS[:3], what=("packed", w, h))
    clip_and_loop(inv, FRAMES[:3], TS[:3], what=("aligned", w, h), **aligned_layout(w, h))
    assert inv.clip_supersampled_batches() == 2


# ---- 3. output layout ----

@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_bytes_per_pixel_and_padded_strides(pond_filter, bpp):
    inv = pond_filter.invoke(W, H)
    inv.set_image("in", F.synthetic_image(W, H, seed=5))
    clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=bpp, what=(bpp, "packed"))
    stride = W * bpp + 5                                     # no multiple of 16 (nor of 4, for bpp 4: the byte kernel)
    assert stride % 16 and (H * stride + 77) % 16
    clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=bpp, row_stride=stride, frame_stride=H * stride + 77, what=(bpp, "padded"))
    stride = W * bpp + 8 - (W * bpp) % 4                     # a multiple of 4 that is no multiple of 16; so is the frame stride
    stride += 4 if stride % 16 == 0 else 0
    clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=bpp, row_stride=stride, frame_stride=H * stride + 4 + (16 if (H * stride + 4) % 16 == 0 else 0),
                  what=(bpp, "padded, dwords"))
    assert inv.clip_supersampled_batches() == 3


@pytest.mark.parametrize("offset", [4, 1], ids=["dword-aligned", "unaligned"])
def test_output_pointer_off_the_16_byte_grid(pond_filter, offset):
    inv = pond_filter.invoke(W, H)
    inv.set_image("in", F.synthetic_image(W, H, seed=5))
    clip_and_loop(inv, FRAMES[:3], TS[:3], offset=offset, what=offset, **aligned_layout(W, H))


@pytest.mark.parametrize("name", ["pond", "wave", "mandelbrot-specialised"])
def test_offset_region(name):
    src, opts = ("mandelbrot", {"specialize": True}) if name == "mandelbrot-specialised" else (WAVE if name == "wave" else name, {})
    flt, inv = make(src, **opts)
    region = (21, 9, 235, 150)
    clip_and_loop(inv, FRAMES[:4], TS[:4], region=region, what=(name, "region"))
    clip_and_loop(inv, FRAMES[:4], TS[:4], region=region, row_stride=235 * 4 + 52, frame_stride=150 * (235 * 4 + 52) + 1000,
                  what=(name, "region, padded"))
    clip_and_loop(inv, FRAMES[:4], TS[:4], region=region, bpp=3, what=(name, "region, bpp 3"))


def test_python_wrapper_returns_the_frames(pond_filter):
    inv = pond_filter.invoke(96, 64)
    inv.set_image("in", F.synthetic_image(96, 64, seed=5))
    want = clip_and_loop(inv, FRAMES[:3], TS[:3])
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3], supersample=True)
    assert got.shape == (3, 64, 96, 4) and got.dtype == np.uint8 and np.array_equal(got, want)
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3], supersample=True, bpp=3, region=(5, 3, 70, 50))
    assert got.shape == (3, 50, 70, 3)
    assert np.array_equal(got, clip_and_loop(inv, FRAMES[:3], TS[:3], bpp=3, region=(5, 3, 70, 50)))
    # num_frames alone: the command line's animation
    got = inv.render_clip(num_frames=4, supersample=True)
    assert np.array_equal(got, clip_and_loop(inv, range(4), [i / 4 for i in range(4)]))


# ---- 4. batches (the variables are read once: child processes) ----

CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from tests.test_gpu_clip_supersample import make, clip_and_loop, FRAMES, TS, WAVE, W, H
out = {}
for name, src in (("pond", "pond"), ("wave", WAVE)):
    flt, inv = make(src)
    clip_and_loop(inv, FRAMES, TS, what=name)
    out[name] = [flt.clip_supersample_plan(W, H, 7), inv.clip_supersampled_batches(), inv.clip_batched_launches()]
    inv.enable_timing(True)
    assert inv.render_clip(frames=FRAMES, ts=TS, supersample=True).shape == (7, H, W, 4)
    out[name] += [len(inv.drain_kernel_ms()), [k for k, ms in inv.drain_native_kernel_ms()]]
print(json.dumps(out))
"""


def run_child(env):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("cap", ["bytes", "frames"])
def test_a_clip_of_several_batches(pond_filter, cap):
    if cap == "bytes":      # room for three frames' slices and a bit: 7 frames are 3 + 3 + 1
        per, env = 3, {"MMHIP_CLIP_SS_BYTES": str(3 * pond_filter.clip_supersample_plan(W, H, 7)["bytes_per_frame"] + 100)}
    else:
        per, env = 2, {"MMHIP_CLIP_MAX_FRAMES": "2"}
    batches = -(-7 // per)
    out = run_child(env)
    assert sorted(out) == ["pond", "wave"]
    for name, (plan, ss_batches, launches, timed, native) in out.items():
        assert plan["batched"] == 1 and plan["frames_per_batch"] == per and plan["batches"] == batches, (name, plan)
        assert ss_batches == plan["batches"], name
        assert launches == 2 * plan["batches"], name
        assert timed == 2 * batches, name                                   # the nested clip calls' pixel entries
        assert native == ["supersample_combine_clip"] * batches, name


# ---- 5. state ----

def plain_render(inv, w, h):
    p = device_filled(w * h * 4)
    try:
        inv.render_rows(p, 0, h)
        inv.sync()
        return device_read(p, w * h * 4)
    finally:
        lib().mmhip_device_free(C.c_void_p(p))


def test_a_sampling_offset_of_the_callers_survives(pond_filter):
    """... a clip, and a clip call that fails: the plain render before and after gives the same bytes."""
    w, h = 96, 64
    inv = pond_filter.invoke(w, h)
    inv.set_image("in", F.synthetic_image(w, h, seed=5))
    centred = plain_render(inv, w, h)
    assert lib().mmhip_set_sampling_offset(inv._h, 0.25, -0.375) == 0
    before = plain_render(inv, w, h)
    assert not np.array_equal(before, centred)
    clip_and_loop(inv, FRAMES[:3], TS[:3])
    assert np.array_equal(plain_render(inv, w, h), before)
    p = device_filled(3 * w * h * 4)
    try:
        assert clip_ss(inv, FRAMES[:3], TS[:3], (0, 0, w, h), p, w * 4, w * h * 4 - 1, 4) != 0
        assert "frame_stride" in mm.api._err()
        inv.sync()
        assert (device_read(p, 3 * w * h * 4) == SENTINEL).all()
    finally:
        lib().mmhip_device_free(C.c_void_p(p))
    assert np.array_equal(plain_render(inv, w, h), before)
    assert inv.clip_supersampled_batches() == 1


def test_single_supersampled_render_before_and_after_a_clip(pond_filter):
    w, h = 96, 64
    inv = pond_filter.invoke(w, h)
    inv.set_image("in", F.synthetic_image(w, h, seed=5))

    def single():
        p = device_filled(w * h * 4)
        try:
            inv.render_supersampled(p, t=0.5, frame=0)
            inv.sync()
            return device_read(p, w * h * 4)
        finally:
            lib().mmhip_device_free(C.c_void_p(p))

    before = single()
    got = clip_and_loop(inv, FRAMES[:3], TS[:3])
    assert np.array_equal(single(), before)
    assert np.array_equal(got[2].reshape(-1), before)           # FRAMES[2], TS[2] = 0, 0.5


@pytest.mark.parametrize("specialize", [False, True], ids=["generic", "specialised"])
def test_a_user_value_changed_between_two_clips(specialize):
    flt, inv = make("pond", 96, 64, specialize=specialize)
    uv = [u for u in flt.uservals if u["kind"] == mm.api.UV_FLOAT][0]
    other = (uv["float_min"] + uv["float_default"]) / 2 if uv["float_default"] != uv["float_min"] else (uv["float_min"] + uv["float_max"]) / 2
    a = clip_and_loop(inv, FRAMES[:3], TS[:3])
    inv.set(uv["name"], other)
    b = clip_and_loop(inv, FRAMES[:3], TS[:3])
    assert not np.array_equal(a, b)
    inv.set(uv["name"], uv["float_default"])
    assert np.array_equal(clip_and_loop(inv, FRAMES[:3], TS[:3]), a)
    assert inv.clip_supersampled_batches() == 3


def test_two_clips_queued_without_a_sync(pond_filter):
    """Both use the invocation's one set of slices: the second call's slice renders wait for the first call's combine."""
    w, h, n = 96, 64, 3
    inv = pond_filter.invoke(w, h)
    inv.set_image("in", F.synthetic_image(w, h, seed=5))
    size = n * w * h * 4
    clips = [([f + k for f in FRAMES[:n]], [t * 0.5 + 0.1 * k for t in TS[:n]]) for k in range(2)]
    ptrs = [device_filled(size) for _ in range(4)]
    try:
        for k, (frames, ts) in enumerate(clips):
            assert clip_ss(inv, frames, ts, (0, 0, w, h), ptrs[k], w * 4, w * h * 4, 4) == 0
        inv.sync()
        for k, (frames, ts) in enumerate(clips):
            loop_ss(inv, frames, ts, (0, 0, w, h), ptrs[2 + k], w * 4, w * h * 4, 4)
        inv.sync()
        got = [device_read(p, size) for p in ptrs]
    finally:
        for p in ptrs:
            lib().mmhip_device_free(C.c_void_p(p))
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
    assert not np.array_equal(got[0], got[1])


# ---- 6. what is not batched, and filters compiled without supersampling ----

@pytest.mark.parametrize("name", ["gauss_direct", "closure_timed_arg"])
def test_native_calls_and_closures_take_the_loop(name):
    flt, inv = make(name, 160, 121)
    assert flt.clip_supersample_plan(160, 121, 3)["batched"] == 0
    clip_and_loop(inv, FRAMES[:3], TS[:3], what=name)
    clip_and_loop(inv, FRAMES[:3], TS[:3], region=(5, 3, 120, 100), what=(name, "region"))
    assert inv.clip_supersampled_batches() == 0 and inv.clip_batched_launches() == 0


def test_filter_compiled_without_supersampling():
    """The single-frame path does not ask how the filter was compiled either: the same bytes."""
    flt, inv = make("pond", supersampling=False)
    clip_and_loop(inv, FRAMES[:3], TS[:3])
    assert inv.clip_supersampled_batches() == 1


# ---- 7. the yardstick itself, against the oracle ----

@pytest.mark.parametrize("name", ["ident", "pond"])
def test_clip_against_the_oracle(name):
    w, h = 96, 64
    img = F.synthetic_image(w, h, seed=5)
    flt, inv = make(name, w, h, image=img)
    got = inv.render_clip(frames=FRAMES[:3], ts=TS[:3], supersample=True)
    assert inv.clip_supersampled_batches() == 1
    cf = CpuFilter(flt.ir_json_raw)
    for i in range(3):
        want = render_supersampled(cf, w, h, images={"in": img}, t=TS[i], frame=FRAMES[i])
        d = np.abs(got[i].astype(int) - want.astype(int))
        print(name, i, "max", int(d.max()), "differ", int((d > 0).sum()), "beyond 1", int((d > 1).sum()))
        EXPECT.check("%s/frame%d" % (name, i), int(d.max()), int((d > 0).sum()), int((d > 1).sum()), total=d.size)


# ---- 8. the command line ----

def test_cli_batches_supersampled_frames(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a + t * 3), frame / 6, 1] end"
    for tag, extra in {"loop": ["--batch-frames=1"], "clip": ["--batch-frames=3"]}.items():
        p = subprocess.run([CLI, "-o", "-F", "5", "-s", "97x61"] + extra + [src, str(tmp_path / (tag + "%d.png"))],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    files = [open(str(tmp_path / ("loop%d.png" % i)), "rb").read() for i in range(5)]
    assert len(set(files)) == 5      # the frames differ
    for i in range(5):
        assert open(str(tmp_path / ("clip%d.png" % i)), "rb").read() == files[i], i
    # ... and -o is not ignored: other bytes than without it
    p = subprocess.run([CLI, "-F", "5", "-s", "97x61", "--batch-frames=3", src, str(tmp_path / "plain%d.png")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert open(str(tmp_path / "plain1.png"), "rb").read() != files[1]


# ---- 9. the two combine kernels on the same random slices ----

@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_combine_kernels_agree_on_random_bytes(bpp):
    """Rendered frames are smooth; pseudo-random slices put every byte value next to every other (the 16-byte store path
    for bpp 4 at widths that are multiples of 4, dword stores at the others, the byte kernel for bpp 1 - 3)."""
    from mathmap_amd._lib import selftest_lib
    ms = (C.c_double * 2)()
    for w, h in ((1, 1), (4, 9), (7, 8), (64, 17), (333, 41), (1024, 10)):
        differ = selftest_lib().mmhip_selftest_combine_ms(w, h, bpp, 3, 1, ms)
        assert differ == 0, (w, h, bpp, differ, selftest_lib().mmhip_selftest_error())
