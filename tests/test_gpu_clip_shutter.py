"""Motion-blurred clips on the GPU (mmhip_render_clip_shutter, k_shutter_combine_clip).

The yardstick is tests/shutter_reference.py: the sub-sample times, a float32 sum in sub-sample order, one float32 product
and tests/fetch_reference.py's pack.  The kernel alone runs on synthetic maps through the self-test entry; end to end,
the sub-samples are single render_rows(floatmap=True) calls of a *second* invocation at the restated times.  Outputs go
into sentinel-filled buffers that are compared whole: float maps by NaN position and bit pattern, bytes as they are."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import mathmap_amd as mm
from mathmap_amd._lib import lib, selftest_lib
from tests import filters as F
from tests import shutter_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mathmap_amd", "mathmap_hip_cli")
f32 = np.float32
SENTINEL = 0xA5
W, H, N, K, SPAN = 97, 61, 3, 4, 0.07
FRAMES = [2, 0, 1]
TS = [0.9, 0.1, 0.5]


# ---- 1. the kernel alone ----

def run_kernel(maps, region_w, bpp=4, floatmap=False, row_stride=None, frame_stride=None, samples_per_pass=0, offset=0, tail=7):
    """maps: float32 [frames, K, rows, render_w, 4].  Returns the whole output buffer (uint8), `offset` sentinel bytes in
    front of frame 0 and `tail` behind the last frame's band."""
    frames, k, rows, render_w, _ = maps.shape
    maps = np.ascontiguousarray(maps, f32)
    stride = row_stride if row_stride is not None else region_w * bpp
    band = rows * 16 * render_w if floatmap else (rows - 1) * stride + region_w * bpp
    fstride = frame_stride if frame_stride is not None else band
    total = offset + (frames - 1) * fstride + band + tail
    out = np.zeros(total, np.uint8)
    rc = selftest_lib().mmhip_selftest_shutter_combine(maps.ctypes.data_as(C.c_void_p), frames, k, rows, region_w, render_w, bpp,
                                                       1 if floatmap else 0, stride, fstride, samples_per_pass, offset,
                                                       out.ctypes.data_as(C.c_void_p), total, SENTINEL, 0, None)
    assert rc == 0, selftest_lib().mmhip_selftest_error()
    return out


def expected_buffer(maps, region_w, bpp=4, floatmap=False, row_stride=None, frame_stride=None, offset=0, tail=7):
    frames, k, rows, render_w, _ = maps.shape
    stride = row_stride if row_stride is not None else region_w * bpp
    band = rows * 16 * render_w if floatmap else (rows - 1) * stride + region_w * bpp
    fstride = frame_stride if frame_stride is not None else band
    want = np.full(offset + (frames - 1) * fstride + band + tail, SENTINEL, np.uint8)
    for i in range(frames):
        px = R.combine(maps[i][:, :, :region_w], bpp=bpp, floatmap=floatmap)      # [rows, region_w, 4 | bpp]
        for r in range(rows):
            at = offset + i * fstride + r * (16 * render_w if floatmap else stride)
            row = np.ascontiguousarray(px[r]).view(np.uint8).reshape(-1)
            want[at:at + row.size] = row
    return want


def same_buffer(got, want, floatmap):
    if not floatmap:
        return np.array_equal(got, want)
    n = got.size // 4 * 4                      # (float-map buffers start aligned: offset 0)
    return R.same_floats(got[:n].view(f32), want[:n].view(f32)) and np.array_equal(got[n:], want[n:])


def pool(k):
    rng = np.random.default_rng(1000 + k)
    return np.concatenate([R.special_pixels(k, rng), rng.uniform(-0.25, 1.25, (1500, k, 4)).astype(f32)])


def synthetic_maps(px, start, frames, rows, render_w):
    """[frames, K, rows, render_w, 4] from the pool of pixels [P, K, 4], beginning at pixel `start` of it."""
    n = frames * rows * render_w
    take = px[(start + np.arange(n)) % len(px)]                       # [n, K, 4]
    return np.ascontiguousarray(take.reshape(frames, rows, render_w, px.shape[1], 4).transpose(0, 3, 1, 2, 4))


WIDTHS = (1, 3, 4, 5, 63, 64, 65, 257)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 17])
def test_the_kernel_alone(k):
    """Every region width with and without columns behind the region, 1, 2 and 7 rows, 1 and 3 frames; float maps, and
    bytes at every bpp packed at offset 0 and with rows padded by 5 bytes at offsets 1 - 3 (bpp 4: the byte path)."""
    px = pool(k)
    start = case = 0
    covered = 0
    for region_w in WIDTHS:
        for render_w in (region_w, region_w + 3):
            for rows in (1, 2, 7):
                for frames in (1, 3):
                    maps = synthetic_maps(px, start, frames, rows, render_w)
                    start += frames * rows * render_w
                    covered = max(covered, frames * rows * render_w)
                    layouts = [dict(floatmap=True), dict(floatmap=True, frame_stride=rows * 16 * render_w + 48)]
                    for bpp in (1, 2, 3, 4):
                        stride = region_w * bpp + 5
                        layouts.append(dict(bpp=bpp))
                        layouts.append(dict(bpp=bpp, row_stride=stride, frame_stride=rows * stride + 3, offset=1 + (case + bpp) % 3))
                    layouts.append(dict(bpp=4, row_stride=region_w * 4 + 8, frame_stride=rows * (region_w * 4 + 8) + 4))      # padded, still words
                    layouts.append(dict(bpp=4, row_stride=region_w * 4 + 5))                                                   # offset 0, rows off the grid
                    for lay in layouts:
                        got = run_kernel(maps, region_w, **lay)
                        want = expected_buffer(maps, region_w, **lay)
                        assert same_buffer(got, want, lay.get("floatmap", False)), (k, region_w, render_w, rows, frames, lay)
                    case += 1
    assert covered >= len(px)            # the largest case holds every pixel of the pool, the special ones included


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 17])
def test_passes_give_the_bits_of_the_single_pass(k):
    px = pool(k)
    for region_w in WIDTHS:
        maps = synthetic_maps(px, 31 * region_w, 3, 2, region_w + 3)
        for lay in [dict(floatmap=True)] + [dict(bpp=b) for b in (1, 2, 3, 4)] + [dict(bpp=4, offset=1)]:
            single = run_kernel(maps, region_w, **lay)
            assert same_buffer(single, expected_buffer(maps, region_w, **lay), lay.get("floatmap", False))
            for per_pass in sorted({1, 2, k - 1}):
                if per_pass >= k:
                    continue
                got = run_kernel(maps, region_w, samples_per_pass=per_pass, **lay)
                assert np.array_equal(got, single), (k, region_w, lay, per_pass)


def test_the_self_test_entry_refuses_a_buffer_that_is_too_small():
    maps = np.zeros((1, 2, 2, 4, 4), f32)
    out = np.zeros(31, np.uint8)
    rc = selftest_lib().mmhip_selftest_shutter_combine(maps.ctypes.data_as(C.c_void_p), 1, 2, 2, 4, 4, 4, 0, 16, 32, 0, 0,
                                                       out.ctypes.data_as(C.c_void_p), 31, SENTINEL, 0, None)
    assert rc != 0 and "bad arguments" in selftest_lib().mmhip_selftest_error().decode()


# ---- 2. end to end ----

ROTATE = """filter rotating (image in)
  c = cos(t * 2); s = sin(t * 2);
  in(xy:[x * c - y * s, x * s + y * c] * 0.9)
end
"""
# an escape-time loop whose centre follows t (pair mode once specialised)
ESCAPE = """filter escape ()
  n = 0; w = x; v = y; ca = x * 1.5 + t; cb = y * 1.5 - t * 0.5;
  while (w * w + v * v < 4) && (n < 9) do
    tt = w * v; u = w * w - v * v + ca; v = tt + tt + cb; w = u; n = n + 1
  end;
  rgba:[n * 0.0625, w * 0.2 + 0.5, v * 0.2 + 0.5, 1]
end
"""
BLUR_T = """stretched filter blur_t (stretched image in)
  b = gaussian_blur(in, 0.04 + t * 0.05, 0.05);
  b(xy)
end
"""
# in(xy, frame) of a sequence, at coordinates that move with t
SEQUENCE_T = """filter seq_t (image in)
  in(xy * 1.2 + xy:[t * 0.3, -0.07], frame)
end
"""
SEQ = np.random.default_rng(7).integers(0, 256, (3, H, W, 4), dtype=np.uint8)
CASES = {
    "rotate": (ROTATE, {}, None),
    "escape": (ESCAPE, {"specialize": True}, None),
    "pond": ("pond", {}, None),
    "blur": (BLUR_T, {}, None),
    "closure": ("closure_timed_arg", {}, None),
    "sequence": (SEQUENCE_T, {}, SEQ),
}


def compiled(name):
    src, opts, image = CASES[name]
    return (F.load(src, **opts) if src in F.NAMES else mm.Filter(src, **opts)), image


def invoke(flt, image, w=W, h=H):
    inv = flt.invoke(w, h)
    if F.image_names(flt):
        inv.set_image("in", F.synthetic_image(w, h, seed=5) if image is None else image)
    return inv


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


def sub_sample_maps(inv, frames, ts, samples, span, region=None, rows=None):
    """float32 [N, K, rows, region_w, 4]: every sub-sample a single render_rows(floatmap=True) at the restated time."""
    rx, ry, rw, rh = region if region is not None else (0, 0, inv.render_width, inv.render_height)
    first, last = rows if rows is not None else (ry, ry + rh)
    times = R.sample_ts(ts, samples, span)
    size = (last - first) * 16 * inv.render_width
    out = np.empty((len(frames), samples, last - first, rw, 4), f32)
    dev = lib().mmhip_device_alloc(size)
    assert dev
    try:
        for i, frame in enumerate(frames):
            for j in range(samples):
                inv.render_rows(dev, first, last, t=float(times[i, j]), frame=int(frame), floatmap=True, region=(rx, ry, rw, rh))
                inv.sync()
                out[i, j] = device_read(dev, size).view(f32).reshape(last - first, inv.render_width, 4)[:, :rw]
    finally:
        lib().mmhip_device_free(C.c_void_p(dev))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_whole_frames_equal_the_restatement(name):
    flt, image = compiled(name)
    inv, other = invoke(flt, image), invoke(flt, image)
    got = inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=K, shutter_span=SPAN)
    assert got.shape == (N, H, W, 4) and got.dtype == np.uint8
    subs = sub_sample_maps(other, FRAMES, TS, K, SPAN)
    for i in range(N):
        assert not R.same_floats(subs[i, 0], subs[i, K - 1]), (name, i, "the sub-samples do not differ: nothing is blurred")
        want = R.combine(subs[i], bpp=4)
        bad = np.argwhere(got[i] != want)
        assert bad.size == 0, (name, i, len(bad), bad[0].tolist())
    assert not np.array_equal(got[0], got[1])
    assert inv.clip_shutter_batches() == 1 and other.clip_shutter_batches() == 0
    if name == "escape":
        assert flt.specialized().clip_launch_geometry(W, H, N * K)["pair_mode"] == 1
    if name in ("rotate", "escape", "pond", "sequence"):
        assert inv.clip_batched_launches() == 1            # the N * K sub-samples of the call: one pixel launch
    if name == "blur":
        assert inv.clip_native_batches() == 1 and inv.clip_batched_launches() == 0
    if name == "closure":
        assert inv.clip_native_batches() == 0 and inv.clip_batched_launches() == 0


@pytest.mark.parametrize("name", ["rotate", "escape"])
def test_bands_regions_formats(name):
    flt, image = compiled(name)
    inv, other = invoke(flt, image), invoke(flt, image)
    region, rows = (11, 7, 70, 41), (13, 40)                     # rows 13 .. 39 of a region that begins at row 7
    rw, nrows = region[2], rows[1] - rows[0]
    subs = sub_sample_maps(other, FRAMES, TS, K, SPAN, region=region, rows=rows)
    for what, bpp, floatmap in (("bytes", 4, False), ("bpp 3", 3, False), ("bpp 1", 1, False), ("floatmap", 4, True)):
        if floatmap:
            stride, row_bytes, row_step = 0, rw * 16, 16 * W
            fstride = nrows * row_step + 80
        else:
            stride = row_step = rw * bpp + 13
            row_bytes, fstride = rw * bpp, nrows * stride + 101
        lead = 64
        total = lead + N * fstride + 64
        want = np.full(total, SENTINEL, np.uint8)
        for i in range(N):
            px = R.combine(subs[i], bpp=bpp, floatmap=floatmap)
            for r in range(nrows):
                at = lead + i * fstride + r * row_step
                want[at:at + row_bytes] = np.ascontiguousarray(px[r]).view(np.uint8).reshape(-1)
        dev = device_filled(total)
        try:
            assert inv.render_clip(frames=FRAMES, ts=TS, out_ptr=dev + lead, rows=rows, region=region, row_stride=stride or None,
                                   frame_stride=fstride, bpp=bpp, floatmap=floatmap, shutter_samples=K, shutter_span=SPAN) is None
            inv.sync()
            got = device_read(dev, total)
        finally:
            lib().mmhip_device_free(C.c_void_p(dev))
        assert same_buffer(got, want, floatmap), (name, what)


# ---- 3. special cases ----

def test_one_sample_is_render_clip():
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    plain = inv.render_clip(frames=FRAMES, ts=TS)
    for span in (SPAN, 0.0, -3.0):
        assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=1, shutter_span=span), plain)
    assert inv.clip_shutter_batches() == 0


@pytest.mark.parametrize("span", [0.0, -0.11])
def test_zero_and_negative_spans(span):
    flt, image = compiled("rotate")
    inv, other = invoke(flt, image), invoke(flt, image)
    got = inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=3, shutter_span=span)
    subs = sub_sample_maps(other, FRAMES, TS, 3, span)
    for i in range(N):
        assert np.array_equal(got[i], R.combine(subs[i], bpp=4)), (span, i)
    if span == 0.0:
        assert R.same_floats(subs[:, 0], subs[:, 2])          # one instant, three times
    else:
        assert R.sample_ts(TS, 3, span)[0, 2] < f32(TS[0])


def test_the_shutter_fraction_of_the_animation():
    flt, image = compiled("rotate")
    inv, other = invoke(flt, image), invoke(flt, image)
    got = inv.render_clip(num_frames=N, shutter_samples=K, shutter=0.5)
    span = f32(np.float64(0.5) / N)
    ts = [f32(i) / f32(N) for i in range(N)]
    subs = sub_sample_maps(other, range(N), ts, K, span)
    for i in range(N):
        assert np.array_equal(got[i], R.combine(subs[i], bpp=4)), i


# ---- 4. batches and passes (the budget is read once: child processes) ----

CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from tests.test_gpu_clip_shutter import compiled, invoke, W, H, SPAN
n, k = int(sys.argv[1]), int(sys.argv[2])
flt, image = compiled("rotate")
inv = invoke(flt, image)
frames, ts = list(range(n)), [0.1 + 0.2 * i for i in range(n)]
out = inv.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=SPAN)
res = {"plan": flt.clip_shutter_plan(W, H, W, k, n), "batches": inv.clip_shutter_batches(), "sha": hashlib.sha256(out.tobytes()).hexdigest()}
inv.enable_timing(True)
again = inv.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=SPAN)
res["again"] = hashlib.sha256(again.tobytes()).hexdigest()
res["native"] = [name for name, ms in inv.drain_native_kernel_ms()]
print(json.dumps(res))
"""


def run_child(n, k, budget):
    env = dict(os.environ, MMHIP_CLIP_SHUTTER_BYTES=str(budget))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(n), str(k)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["three batches", "carry"])
def test_batches_and_passes_leave_the_bytes_alone(case):
    bps = H * 16 * W
    if case == "three batches":                 # room for two frames of 4 sub-samples: 5 frames are 2 + 2 + 1
        n, k, budget, want = 5, 4, 8 * bps + 100, dict(frames_per_batch=2, batches=3, samples_per_pass=4, passes=1, carry=0)
    else:                                       # three maps: two sub-samples per pass beside the carry, 5 are 2 + 2 + 1
        n, k, budget, want = 1, 5, 3 * bps, dict(frames_per_batch=1, batches=1, samples_per_pass=2, passes=3, carry=1)
    res = run_child(n, k, budget)
    assert dict(res["plan"], bytes_per_sample=bps) == dict(want, bytes_per_sample=bps), res["plan"]
    assert res["batches"] == want["batches"]
    assert res["native"] == ["shutter_combine_clip"] * (want["batches"] * want["passes"])
    # this process has the default budget: one batch, one pass
    flt, image = compiled("rotate")
    inv = invoke(flt, image)
    assert flt.clip_shutter_plan(W, H, W, k, n)["batches"] == 1 and flt.clip_shutter_plan(W, H, W, k, n)["passes"] == 1
    here = inv.render_clip(frames=list(range(n)), ts=[0.1 + 0.2 * i for i in range(n)], shutter_samples=k, shutter_span=SPAN)
    sha = hashlib.sha256(here.tobytes()).hexdigest()
    assert res["sha"] == sha and res["again"] == sha


# ---- 5. state ----

@pytest.mark.parametrize("name", ["rotate", "blur"])
def test_renders_around_a_shutter_clip(name):
    flt, image = compiled(name)
    inv, fresh = invoke(flt, image), invoke(flt, image)
    want = fresh.render(t=0.3, frame=1)
    assert np.array_equal(inv.render(t=0.3, frame=1), want)
    clip_before = inv.render_clip(frames=FRAMES, ts=TS)
    blurred = inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=K, shutter_span=SPAN)
    assert not np.array_equal(blurred, clip_before)
    assert np.array_equal(inv.render(t=0.3, frame=1), want)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS), clip_before)
    assert np.array_equal(inv.render_clip(frames=FRAMES, ts=TS, shutter_samples=K, shutter_span=SPAN), blurred)


@pytest.mark.parametrize("mode", ["maps", "fused"])
def test_the_shutter_clip_renders_at_the_callers_sampling_offset(mode):
    """A motion-blurred clip has one sample per pixel and instant: it is taken at the invocation's sampling offset, as
    every single render is, and the offset is still there afterwards.  (The grid of render_clip(aa=...) replaces it:
    tests/test_gpu_clip_sampled.py.)"""
    w = h = 17
    frames, ts, k, offset = [2, 0], [0.9, 0.1], 3, (-0.5, 0.25)
    flt, image = compiled("rotate")
    inv, other, fresh, centred = (invoke(flt, image, w, h) for _ in range(4))
    for i in (inv, other, fresh):
        i.set_sampling_offset(*offset)
    got = inv.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=SPAN, shutter_mode=mode)
    subs = sub_sample_maps(other, frames, ts, k, SPAN)          # six single renders at the offset
    for i in range(len(frames)):
        assert np.array_equal(got[i], R.combine(subs[i], bpp=4)), (mode, i)
    assert not np.array_equal(got, centred.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=SPAN, shutter_mode=mode))
    assert (inv.clip_shutter_fused_batches(), inv.clip_shutter_batches()) == ((1, 0) if mode == "fused" else (0, 1))
    assert np.array_equal(inv.render(t=0.3, frame=1), fresh.render(t=0.3, frame=1))
    assert not np.array_equal(inv.render(t=0.3, frame=1), centred.render(t=0.3, frame=1))


# ---- 6. the command line ----

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


def test_cli_writes_the_python_result(tmp_path):
    src = "filter swirl (float k: 0-8 (3)) rgba:[0.5 + 0.5 * sin(k * r + t * 6), 0.5 + 0.5 * cos(a + t * 3), frame / 6, 1] end"
    want = mm.Filter(src).invoke(W, H).render_clip(num_frames=3, shutter_samples=4, shutter=0.5)
    for tag, extra in (("one", []), ("two", ["--batch-frames=2"])):
        p = subprocess.run([CLI, "-F", "3", "--shutter-samples=4", "--shutter=0.5", "-s", "%dx%d" % (W, H)] + extra +
                           [src, str(tmp_path / (tag + "%d.png"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        for i in range(3):
            assert np.array_equal(read_png(str(tmp_path / ("%s%d.png" % (tag, i)))), want[i, :, :, :3]), (tag, i)
    # ... and the options are not ignored: other bytes than without them
    p = subprocess.run([CLI, "-F", "3", "-s", "%dx%d" % (W, H), src, str(tmp_path / "plain%d.png")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert not np.array_equal(read_png(str(tmp_path / "plain1.png")), want[1, :, :, :3])


# ---- 7. one size test ----

def test_full_hd():
    w, h, n, k = 1920, 1080, 2, 4
    flt, image = compiled("rotate")
    inv, other = invoke(flt, image, w, h), invoke(flt, image, w, h)
    frames, ts = [0, 1], [0.2, 0.7]
    got = inv.render_clip(frames=frames, ts=ts, shutter_samples=k, shutter_span=0.05)
    subs = sub_sample_maps(other, frames, ts, k, 0.05)
    for i in range(n):
        assert np.array_equal(got[i], R.combine(subs[i], bpp=4)), i
    assert inv.clip_shutter_batches() == 1
